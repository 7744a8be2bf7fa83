"""GPU suite: the backward of the DPV fusion (csrc/dpv_fuse_bwd.hip behind ops.dpv_fuse) against torch autograd in float64 on
the composition of models/models.py:666-672 with utils/img_utils.py:31-47, :360-375, written out below; nmode
"default_upsample" of BaseModel trains against a torch twin and runs through BaseLoss.

Gradient parity prints, per case, max |g_hip - g64| on the kept pixels next to E_ref, the float32 torch composition's own error
there (on the CPU 2.9e-6 ... 3.7e-6 with g_l present, 2e-7 of max |g64|); the bound is max(8 E_ref, 4e-5 max |g64|), the second
term from the 7e-6 relative error of the forward's hardware exp2 / log2 helpers at |x + log m| up to |log eps| = 36."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pdepth_amd
from pdepth_amd import ops, synth
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

VAR = 0.3
EPS = torch.finfo(float).eps
SHAPES = [(2, 64, 16, 24),    # register form, full
          (2, 48, 9, 37),     # register form with D < 64; 333 pixels is not a multiple of 256
          (1, 130, 8, 20)]    # re-reading form
MODES = ["g_f", "g_l", "both"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def fuse_torch(logp, dmaps, masks, dc, var=VAR, eps=EPS):
    """(q, fused, log fused) in the dtype of logp: gen_soft_label_torch(zero_invalid=True) blended with the uniform DPV by the
    mask and clamped (utils/img_utils.py:31-47, :371, :374), multiplied into the DPV, renormalised, clamped, log
    (models/models.py:666-672).  q is the posterior before the clamp."""
    dt = logp.dtype
    d = dc.to(dt).view(1, -1, 1, 1)
    sigma = torch.sqrt(torch.tensor(var, dtype=dt, device=logp.device))
    dists = torch.exp(-torch.pow(torch.abs(d - dmaps.to(dt).unsqueeze(1)), 2.0) / (2 * torch.pow(sigma, 2.0)))
    dists = dists / torch.sum(dists, dim=1, keepdim=True)
    dists = torch.where(dists != dists, torch.full_like(dists, -1.0), dists)
    mask = masks.to(dt).unsqueeze(1)
    tofuse = torch.clamp(dists * mask + (1.0 / d.shape[1]) * (1.0 - mask), eps, 1.0)
    u = torch.exp(logp + torch.log(tofuse))
    q = u / torch.sum(u, dim=1, keepdim=True)
    fused = torch.clamp(q, eps, 1.0)
    return q, fused, torch.log(fused)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    B, D, H, W = shape
    g = torch.Generator().manual_seed(11)
    logp = F.log_softmax(3 * torch.randn(B, D, H, W, generator=g), dim=1)
    dmaps = 3 + 39 * torch.rand(B, H, W, generator=g)
    dmaps[0, 0, :4] = 1000.0          # every Gaussian underflows: the NaN -> -1 branch
    masks = (torch.rand(B, H, W, generator=g) < 0.5).float()
    g_f = torch.randn(B, D, H, W, generator=g)
    g_l = torch.randn(B, D, H, W, generator=g)
    return logp, dmaps, masks, synth.powerf(5, 40, D, 1.0), g_f, g_l


def _on(dev, shape):
    logp, dmaps, masks, dc, g_f, g_l = _inputs(shape)
    return logp.to(dev), dmaps.to(dev), masks.to(dev), dc, g_f.to(dev), g_l.to(dev)


def _torch_grad(logp, dmaps, masks, dc, g_f, g_l, dtype):
    """(gradient with respect to logp, q) of the composition evaluated in `dtype`."""
    x = logp.to(dtype).detach().clone().requires_grad_(True)
    dct = torch.as_tensor(np.asarray(dc, dtype=np.float32)).to(x.device)   # the candidates the kernels see: fp32 values
    q, fused, logf = fuse_torch(x, dmaps, masks, dct)
    total = 0
    if g_f is not None:
        total = total + (fused * g_f.to(dtype)).sum()
    if g_l is not None:
        total = total + (logf * g_l.to(dtype)).sum()
    total.backward()
    return x.grad, q.detach()


_ORACLE = {}


def _oracle(dev, shape, mode):
    """(g64, g32, kept pixels [B,H,W], share of clamped planes): computed once per case, never modified."""
    key = (shape, mode)
    if key not in _ORACLE:
        logp, dmaps, masks, dc, g_f, g_l = _on(dev, shape)
        gf, gl = (g_f if mode != "g_l" else None), (g_l if mode != "g_f" else None)
        g64, q64 = _torch_grad(logp, dmaps, masks, dc, gf, gl, torch.float64)
        g32, _ = _torch_grad(logp, dmaps, masks, dc, gf, gl, torch.float32)
        kept = ~((q64 / EPS - 1).abs() < 1e-3).any(dim=1)
        _ORACLE[key] = (g64, g32, kept, float((q64 < EPS).double().mean()))
    return _ORACLE[key]


def _hip_grad(logp, dmaps, masks, dc, g_f, g_l, **kw):
    x = logp.detach().clone().requires_grad_(True)
    fused, logf = ops.dpv_fuse(x, dmaps, masks, dc, var=VAR, **kw)
    total = 0
    if g_f is not None:
        total = total + (fused * g_f).sum()
    if g_l is not None:
        total = total + (logf * g_l).sum()
    total.backward()
    return x.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_parity(dev, shape, mode):
    logp, dmaps, masks, dc, g_f, g_l = _on(dev, shape)
    g64, g32, kept, clamped = _oracle(dev, shape, mode)
    g = _hip_grad(logp, dmaps, masks, dc, g_f if mode != "g_l" else None, g_l if mode != "g_f" else None)
    excluded = 1.0 - float(kept.double().mean())
    assert excluded <= 0.02, excluded
    k = kept.unsqueeze(1).expand_as(g64)
    scale = float(g64[k].abs().max())
    e_ref = float((g32.double() - g64)[k].abs().max())
    err = float((g.double() - g64)[k].abs().max())
    print(f"fuse backward {shape} {mode}: max|g_hip - g64| = {err:.3e} ({err / scale:.2e} of max|g64| = {scale:.3e}), "
          f"E_ref = {e_ref:.3e} ({e_ref / scale:.2e}), excluded pixels {100 * excluded:.2f} %, clamped planes {100 * clamped:.1f} %")
    assert torch.isfinite(g[k]).all()
    assert err <= max(8 * e_ref, 4e-5 * scale), (err, e_ref, scale)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_under_autograd_is_bit_identical(dev, shape):
    logp, dmaps, masks, dc, _, _ = _on(dev, shape)
    before = logp.clone()
    plain = ops.dpv_fuse(logp, dmaps, masks, dc, var=VAR)
    under = ops.dpv_fuse(logp.clone().requires_grad_(True), dmaps, masks, dc, var=VAR)
    assert torch.equal(plain[0], under[0]) and torch.equal(plain[1], under[1])
    assert under[0].requires_grad and under[1].requires_grad and not plain[0].requires_grad
    assert torch.equal(logp, before)
    with torch.no_grad():   # grad mode off: today's path, nothing recorded
        off = ops.dpv_fuse(logp.clone().requires_grad_(True), dmaps, masks, dc, var=VAR)
    assert torch.equal(plain[0], off[0]) and not off[0].requires_grad


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reproducible(dev, shape):
    args = _on(dev, shape)
    assert torch.equal(_hip_grad(*args), _hip_grad(*args))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_non_finite_stays_in_its_pixel(dev, shape):
    logp, dmaps, masks, dc, g_f, g_l = _on(dev, shape)
    clean = _hip_grad(logp, dmaps, masks, dc, g_f, g_l)
    bad = logp.clone()
    b, k, y, x = shape[0] - 1, shape[1] // 2, shape[2] // 2, shape[3] // 3
    bad[b, k, y, x] = float("nan")
    g = _hip_grad(bad, dmaps, masks, dc, g_f, g_l)
    assert not torch.isfinite(g[b, :, y, x]).any()
    other = torch.ones(shape[0], shape[2], shape[3], dtype=torch.bool, device=dev)
    other[b, y, x] = False
    o = other.unsqueeze(1).expand_as(g)
    assert torch.equal(g[o], clean[o])


def test_partial_requests(dev):
    shape = SHAPES[1]
    logp, dmaps, masks, dc, g_f, g_l = _on(dev, shape)
    for mode, kw in (("g_l", dict(want_fused=False)), ("g_f", dict(want_log=False))):
        x = logp.detach().clone().requires_grad_(True)
        fused, logf = ops.dpv_fuse(x, dmaps, masks, dc, var=VAR, **kw)
        assert (fused is None) == (mode == "g_l") and (logf is None) == (mode == "g_f")
        ((logf * g_l) if fused is None else (fused * g_f)).sum().backward()
        both_outputs = _hip_grad(logp, dmaps, masks, dc, g_f if mode == "g_f" else None, g_l if mode == "g_l" else None)
        assert torch.equal(x.grad, both_outputs)
        g64, g32, kept, _ = _oracle(dev, shape, mode)
        k = kept.unsqueeze(1).expand_as(g64)
        scale = float(g64[k].abs().max())
        assert float((x.grad.double() - g64)[k].abs().max()) <= max(8 * float((g32.double() - g64)[k].abs().max()), 4e-5 * scale)
    # no gradient into either output: the Function answers None without a launch
    assert ops._DpvFuseFn.backward(None, None, None) == (None,) * 8


def test_refusals(dev):
    logp, dmaps, masks, dc, _, _ = _on(dev, SHAPES[0])
    x = logp.clone().requires_grad_(True)
    dct = torch.tensor(np.asarray(dc), dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match="dpv_fuse: dmaps requires grad"):
        ops.dpv_fuse(x, dmaps.clone().requires_grad_(True), masks, dc)
    with pytest.raises(RuntimeError, match="dpv_fuse: masks requires grad"):
        ops.dpv_fuse(x, dmaps, masks.clone().requires_grad_(True), dc)
    with pytest.raises(RuntimeError, match="dpv_fuse: d_candi requires grad"):
        ops.dpv_fuse(x, dmaps, masks, dct.clone().requires_grad_(True))
    fused, _ = ops.dpv_fuse(x, dmaps, masks, dct)   # a tensor d_candi that is data is fine
    assert fused.requires_grad


# ---- BaseModel, nmode default_upsample, trains -----------------------------------------------------------------------------
# torch stand-ins of the HIP ops for the twin (the first four as in tests/test_sweep_backward.py)
def _torch_sweep_cost(ref, src, K, R, t, rays, cxcy, d_candi, sigma, feat_dist="L2", algo="auto", blas=None):
    B, V, C, H, W = src.shape
    dc = ops.d_candi_tensor(d_candi, ref.device)
    D = dc.numel()
    out = []
    for i in range(B):
        cost = 0
        for v in range(V):
            grid = O.plane_coords(K[i], R[i, v], t[i, v], rays[i], dc, cxcy[i, 0], cxcy[i, 1]).reshape(D, H, W, 2)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                                   align_corners=False)
            cost = cost + ((warped - ref[i].unsqueeze(0)) ** 2).sum(1) / sigma
        out.append(cost)
    return torch.stack(out)


def _torch_dpv_reduce_ex(logits, d_candi=None, addend=None, want_logp=True, want_prob=False, want_depth=False, want_var=False,
                         want_quarter=False, inplace=False):
    x = logits if addend is None else logits + addend
    logp = F.log_softmax(x, dim=1)
    out = {"logp": logp}
    if want_prob:
        out["prob"] = torch.exp(logp)
    if want_depth:
        out["depth"] = (torch.exp(logp) * ops.d_candi_tensor(d_candi, x.device).view(1, -1, 1, 1)).sum(1)
    if want_quarter:
        out["quarter"] = F.interpolate(logp.detach(), scale_factor=0.25, mode="nearest")
    return out


def _torch_dpv_reduce(logits, d_candi, want_logp=True, want_depth=True, inplace=False):
    r = _torch_dpv_reduce_ex(logits, d_candi, want_depth=want_depth)
    return r["logp"], r.get("depth")


def _torch_dpv_expect(dpv, d_candi, BV_log=False):
    z = torch.exp(dpv) if BV_log else dpv
    return (z * ops.d_candi_tensor(d_candi, dpv.device).view(1, -1, 1, 1)).sum(1)


def _torch_dpv_fuse(logp, dmaps, masks, d_candi, var=0.3, eps=None, want_fused=True, want_log=True):
    if masks.dim() == 4:
        masks = masks[:, 0]
    _, fused, logf = fuse_torch(logp, dmaps.float(), masks.float(), ops.d_candi_tensor(d_candi, logp.device), var,
                                EPS if eps is None else eps)
    return (fused if want_fused else None), (logf if want_log else None)


def _model_loss(model, inp, target):
    out = model([inp])[0]
    d = inp["d_candi"]
    loss = 0
    for bv in out["output"] + out["output_refined"]:
        depth = ops.dpv_expect(bv, d, BV_log=True)
        tgt = F.interpolate(target.unsqueeze(1), size=depth.shape[-2:], mode="nearest").squeeze(1)
        loss = loss + (depth - tgt).abs().mean()
    return loss


def _upsample_input(seed, B, H, W, dev, gen):
    inp = synth.make_model_input(seed, B=B, V=1, H=H, W=W, D=64, pose="mono")
    masks = (torch.rand(B, 1, H // 4, W // 4, generator=gen) > 0.7).float()
    inp["dmaps"] = (torch.rand(B, H // 4, W // 4, generator=gen) * 30 + 6) * masks[:, 0]
    inp["masks"] = masks
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def _upsample_model(dev, cfg):
    from pdepth_amd.models.get_model import get_model
    torch.manual_seed(0)
    model = get_model(cfg, 0)
    synth.seed_weights(model, seed=31)
    return model.to(dev).train()


def test_upsample_model_trains(dev, monkeypatch):
    model = _upsample_model(dev, synth.default_cfg("default_upsample"))
    inp = _upsample_input(3100, 2, 256, 256, dev, torch.Generator().manual_seed(1))
    target = torch.rand(2, 256, 256, generator=torch.Generator().manual_seed(2)).to(dev) * 30 + 5
    twin = copy.deepcopy(model)
    loss = _model_loss(model, inp, target)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads and all(torch.isfinite(g).all() for g in grads.values())
    with monkeypatch.context() as mp:
        mp.setattr(ops, "sweep_cost", _torch_sweep_cost)
        mp.setattr(ops, "dpv_reduce_ex", _torch_dpv_reduce_ex)
        mp.setattr(ops, "dpv_reduce", _torch_dpv_reduce)
        mp.setattr(ops, "dpv_expect", _torch_dpv_expect)
        mp.setattr(ops, "dpv_fuse", _torch_dpv_fuse)
        tloss = _model_loss(twin, inp, target)
        tloss.backward()
    print("default_upsample: loss", float(loss), "twin", float(tloss))
    assert abs(float(loss) - float(tloss)) <= 1e-3 * abs(float(tloss))
    checked = 0
    for n, p in twin.named_parameters():
        if not (n.startswith("base_encoder") or n.startswith("conv0") or n.startswith("base_decoder")) or p.grad is None:
            continue
        g, gt = grads[n], p.grad
        den = float(gt.norm())
        if den == 0:
            continue
        assert float((g - gt).norm()) <= 1e-3 * den, n
        checked += 1
    assert checked > 10
    # a few SGD steps on a fixed batch lower the loss
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    first = None
    for _ in range(4):
        opt.zero_grad()
        l = _model_loss(model, inp, target)
        first = float(l) if first is None else first
        l.backward()
        opt.step()
    assert float(_model_loss(model, inp, target)) < first


def test_base_loss_on_the_upsample_output(dev):
    from pdepth_amd.losses.get_loss import get_loss
    cfg = synth.default_loss_cfg("default_upsample", loss_name="base")
    model = _upsample_model(dev, cfg)
    B, H, W = 1, 256, 256
    gen = torch.Generator().manual_seed(4)
    T = torch.eye(4)
    T[0, 3] = -0.54
    inputs, targets = [], []
    for seed in (3100, 3101):
        inp = _upsample_input(seed, B, H, W, dev, gen)
        dc = ops.d_candi_tensor(inp["d_candi"], dev).view(1, -1, 1, 1)
        coarse = 8.0 + 28.0 * torch.rand(B, 1, H // 32, W // 32, generator=gen)
        dmap = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0].to(dev)
        mask = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float().to(dev)
        label = lambda d: torch.softmax(-(dc - d.unsqueeze(1)) ** 2 / (2 * 0.3), dim=1)
        K_up = inp["intrinsics"].clone()
        K_up[:, :2] *= 4.0
        targets.append({"d_candi": inp["d_candi"], "T_left2right": T, "rgb": inp["rgb"], "intrinsics": inp["intrinsics"],
                        "intrinsics_up": K_up, "masks_imgsizes": mask, "masks": mask[:, :, ::4, ::4].contiguous(),
                        "soft_labels_imgsize": label(dmap), "soft_labels": label(dmap[:, ::4, ::4].contiguous())})
        inputs.append(inp)
    output = tuple(model(inputs))
    assert len(output[0]["output"]) == 2 and len(output[1]["output"]) == 2
    loss = get_loss(cfg, 0)(output, tuple(targets))
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    print("BaseLoss on default_upsample:", float(loss))
    assert bool(torch.isfinite(loss)) and len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
