"""GPU suite of the training loss: ops.dpv_soft_ce (csrc/loss.hip) against a float64 evaluation of its formula and the
reference's values (fixture g24), its two label forms, its depth output, determinism, the item without a valid pixel, the
refusals; BaseLoss against the reference's BaseLoss.forward (fixture g24), without a host synchronisation, and end to end
behind BaseModel."""
import os

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import ops, synth
from pdepth_amd.losses import get_loss
from pdepth_amd.losses.losses import BaseLoss
from pdepth_amd.utils import img_utils
from util import golden
import util_loss as U

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |loss - loss64| <= 1e-5 |loss64|: every summand -label logp mask is non-negative on valid pixels, so a tree reduction over
# D H W <= 2^23 terms has a relative error of at most ~23 * 2^-24 = 1.4e-6; the bound leaves 7x.
LOSS_RTOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _case(seed, B, D, H, W, dev, mask_kind="binary"):
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(2 * torch.randn(B, D, H, W, generator=g, dtype=torch.float64), 1).float()
    label = torch.softmax(3 * torch.randn(B, D, H, W, generator=g, dtype=torch.float64), 1).float()
    mask = (torch.rand(B, H, W, generator=g) < 0.6).float()
    if mask_kind == "values":
        mask[:, 0, :3] = 0.5
    dc = synth.powerf(5.0, 40.0, D, 1.0)
    return logp.to(dev), label.to(dev), mask.to(dev), dc


def _ce64(logp, label, mask):
    """The formula in float64 -> loss [B] (0 where no mask entry equals one); differentiable with respect to logp."""
    ce = -(label.double() * logp).sum(1)
    if mask is None:
        return ce.mean((1, 2))
    m = mask.double()
    cnt = (m == 1).sum((1, 2)).double()
    tot = torch.where(m != 0, ce * m, torch.zeros_like(ce)).sum((1, 2))
    return torch.where(cnt > 0, tot / cnt.clamp(min=1), torch.zeros_like(tot))


def _check_loss(loss, want, what):
    loss, want = loss.detach().double().cpu(), want.detach().double().cpu()
    err = (loss - want).abs() / want.abs().clamp(min=1e-300)
    print(what, "loss", loss.tolist(), "float64", want.tolist(), "relative error", err.tolist())
    assert bool(((loss - want).abs() <= LOSS_RTOL * want.abs()).all()), (what, err.tolist())


def _check_grad(g, want, rtol, what):
    g, want = g.double().cpu(), want.double().cpu()
    atol = 1e-6 * float(want.abs().max())
    worst = float(((g - want).abs() - rtol * want.abs()).max())
    print(what, "gradient: max (|g - g64| - rtol |g64|) =", worst, "atol", atol)
    assert torch.allclose(g, want, rtol=rtol, atol=atol), what


@pytest.mark.parametrize("shape", [(2, 64, 64, 96), (1, 64, 256, 384), (2, 20, 7, 9), (1, 128, 16, 32), (1, 130, 8, 8)])
@pytest.mark.parametrize("mask_kind", ["binary", "values", "none"])
def test_label_form_against_float64(dev, shape, mask_kind):
    logp, label, mask, dc = _case(11 + shape[1], *shape, dev, mask_kind)
    mask = None if mask_kind == "none" else mask
    x = logp.clone().requires_grad_(True)
    loss, depth = ops.dpv_soft_ce(x, dc, label=label, mask=mask)
    assert depth is None and loss.shape == (shape[0],)
    x64 = logp.double().requires_grad_(True)
    want = _ce64(x64, label, mask)
    _check_loss(loss, want, f"{shape} {mask_kind}")
    w = torch.arange(1, shape[0] + 1, device=dev, dtype=torch.float32)
    (loss * w).sum().backward()
    (want * w.double()).sum().backward()
    _check_grad(x.grad, x64.grad, 1e-5, f"{shape} {mask_kind}")


def test_label_form_against_the_reference(dev):
    g = golden("g24_loss.npz")
    inp = U.make_inputs()
    for s in U.SIDES:
        x = torch.from_numpy(inp[f"logp_{s}_lo"]).to(dev).requires_grad_(True)
        label = torch.from_numpy(g[f"label_{s}_lo"]).to(dev)
        for tag, mask in (("", torch.from_numpy(inp[f"mask_{s}_lo"]).to(dev)), ("_zero", torch.zeros(U.B, 1, *U.LO, device=dev))):
            x.grad = None
            loss, _ = ops.dpv_soft_ce(x, U.d_candi(), label=label, mask=mask)
            loss.sum().backward()
            want = torch.tensor([float(g[f"ce{tag}_{s}_{i}"]) for i in range(U.B)])
            want_g = torch.from_numpy(np.concatenate([g[f"ce{tag}_grad_{s}_{i}"] for i in range(U.B)]))
            _check_loss(loss, want, f"g24 {s}{tag}")
            _check_grad(x.grad, want_g, 1e-5, f"g24 {s}{tag}")
            if tag == "_zero":
                assert float(loss.abs().max()) == 0.0 and float(x.grad.abs().max()) == 0.0
    assert float(g["ce_left_1"]) == 0.0   # (the item whose mask has no entry equal to one)


@pytest.mark.parametrize("shape", [(2, 64, 64, 96), (2, 20, 7, 9)])
def test_from_depth_form_equals_label_form(dev, shape):
    B, D, H, W = shape
    logp, _, mask, dc = _case(5, *shape, dev)
    g = torch.Generator().manual_seed(6)
    depth_gt = 5.0 + 35.0 * torch.rand(B, H, W, generator=g)
    depth_gt[0, 1, :4] = 40.0 + 20.0   # every Gaussian underflows to 0: label -1 on every plane
    mask[0, 1, :4] = 0.0
    var = torch.tensor(0.3)
    label = torch.stack([img_utils.gen_soft_label_torch(dc, depth_gt[i], var, zero_invalid=True) for i in range(B)])
    assert bool((label[0, :, 1, :4] == -1).all())
    depth_gt, label = depth_gt.to(dev), label.to(dev)
    xa, xb = logp.clone().requires_grad_(True), logp.clone().requires_grad_(True)
    la, _ = ops.dpv_soft_ce(xa, dc, label=label, mask=mask)
    lb, _ = ops.dpv_soft_ce(xb, dc, depth_gt=depth_gt, variance=0.3, mask=mask)
    _check_loss(lb, la, f"from depth {shape}")
    la.sum().backward()
    lb.sum().backward()
    _check_grad(xb.grad, xa.grad, 2e-5, f"from depth {shape}")
    assert float(xb.grad[0, :, 1, :4].abs().max()) == 0.0
    # the invalid pixels alone, under their zero mask, and unmasked: label -1
    only = torch.zeros_like(mask)
    x = logp.clone().requires_grad_(True)
    l0, _ = ops.dpv_soft_ce(x, dc, depth_gt=depth_gt, variance=0.3, mask=only)
    l0.sum().backward()
    assert float(l0.abs().max()) == 0.0 and float(x.grad.abs().max()) == 0.0
    only[0, 1, :4] = 1.0
    l1, _ = ops.dpv_soft_ce(logp, dc, depth_gt=depth_gt, variance=0.3, mask=only)
    want = logp[0, :, 1, :4].double().sum() / 4
    assert abs(float(l1[0]) - float(want)) <= LOSS_RTOL * abs(float(want)) and float(l1[1]) == 0.0


@pytest.mark.parametrize("shape", [(2, 64, 64, 96), (2, 20, 7, 9), (1, 130, 8, 8), (1, 128, 16, 32)])
def test_depth_output_is_dpv_expect(dev, shape):
    logp, label, mask, dc = _case(7, *shape, dev)
    loss, depth = ops.dpv_soft_ce(logp, dc, label=label, mask=mask, want_depth=True)
    assert torch.equal(depth, ops.dpv_expect(logp, dc, BV_log=True))
    assert torch.equal(loss, ops.dpv_soft_ce(logp, dc, label=label, mask=mask)[0])
    gd = torch.randn(depth.shape, generator=torch.Generator().manual_seed(8)).to(dev)
    xs = [logp.clone().requires_grad_(True) for _ in range(3)]
    l, d = ops.dpv_soft_ce(xs[0], dc, label=label, mask=mask, want_depth=True)
    (l.sum() + (d * gd).sum()).backward()
    ops.dpv_soft_ce(xs[1], dc, label=label, mask=mask)[0].sum().backward()
    (ops.dpv_expect(xs[2], dc, BV_log=True) * gd).sum().backward()
    both = xs[1].grad + xs[2].grad
    assert torch.allclose(xs[0].grad, both, rtol=1e-6, atol=1e-6 * float(both.abs().max()))


def test_deterministic(dev):
    logp, label, mask, dc = _case(9, 2, 64, 256, 384, dev)
    depth_gt = (5.0 + 35.0 * torch.rand(2, 256, 384, generator=torch.Generator().manual_seed(1))).to(dev)
    for src in (dict(label=label), dict(depth_gt=depth_gt, variance=0.3)):
        runs = []
        for _ in range(2):
            x = logp.clone().requires_grad_(True)
            loss, depth = ops.dpv_soft_ce(x, dc, mask=mask, want_depth=True, **src)
            (loss.sum() + depth.sum()).backward()
            runs.append((loss.detach(), x.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_item_without_valid_pixel(dev):
    logp, label, mask, dc = _case(10, 2, 64, 64, 96, dev)
    mask[1] = 0.0
    logp[1, 3] = float("-inf")   # where the label is 0: 0 * -inf must not leak out of a masked-out pixel
    label[1, 3] = 0.0
    x = logp.clone().requires_grad_(True)
    loss, _ = ops.dpv_soft_ce(x, dc, label=label, mask=mask)
    loss.sum().backward()
    assert float(loss[1]) == 0.0 and float(loss[0]) > 0 and bool(torch.isfinite(loss).all())
    assert float(x.grad[1].abs().max()) == 0.0 and bool(torch.isfinite(x.grad).all())
    x = logp.clone().requires_grad_(True)
    loss, _ = ops.dpv_soft_ce(x, dc, depth_gt=torch.full((2, 64, 96), 20.0, device=dev), variance=0.3, mask=mask)
    loss.sum().backward()
    assert float(loss[1]) == 0.0 and float(x.grad[1].abs().max()) == 0.0 and bool(torch.isfinite(x.grad).all())


def test_forward_values_and_refusals(dev):
    logp, label, mask, dc = _case(12, 2, 64, 64, 96, dev)
    depth_gt = torch.full((2, 64, 96), 20.0, device=dev)
    plain = ops.dpv_soft_ce(logp, dc, label=label, mask=mask, want_depth=True)
    under = ops.dpv_soft_ce(logp.clone().requires_grad_(True), dc, label=label, mask=mask, want_depth=True)
    assert torch.equal(plain[0], under[0]) and torch.equal(plain[1], under[1]) and under[0].requires_grad
    x = logp.clone().requires_grad_(True)
    dct = torch.tensor(dc, dtype=torch.float32, device=dev)
    for name, kw in (("label", dict(label=label.clone().requires_grad_(True))),
                     ("depth_gt", dict(depth_gt=depth_gt.clone().requires_grad_(True), variance=0.3)),
                     ("mask", dict(label=label, mask=mask.clone().requires_grad_(True)))):
        with pytest.raises(RuntimeError, match=f"dpv_soft_ce: {name} requires grad"):
            ops.dpv_soft_ce(x, dc, **kw)
    with pytest.raises(RuntimeError, match="dpv_soft_ce: d_candi requires grad"):
        ops.dpv_soft_ce(x, dct.clone().requires_grad_(True), label=label)
    with pytest.raises(RuntimeError, match="exactly one label source"):
        ops.dpv_soft_ce(logp, dc)


def _fixture_run(dev, labels_from_depth=False, with_labels=True):
    inp = U.make_inputs()
    output, target = U.structure(inp, img_utils.gen_soft_label_torch, dev=dev, with_labels=with_labels)
    crit = BaseLoss(U.loss_cfg(), 0, labels_from_depth=labels_from_depth)
    loss = crit(output, target)
    return loss, output, target, crit


def test_base_loss_against_the_reference(dev):
    g = golden("g24_loss.npz")
    loss, output, _, _ = _fixture_run(dev)
    loss.backward()
    want = float(g["base_loss"])
    print("BaseLoss", float(loss), "reference", want, "reference in float64", float(g["base_loss64"]))
    for name, v in zip(("left_lo", "left_hi", "right_lo", "right_hi"), U.volumes(output)):
        got, ref = v.grad.double().cpu(), torch.from_numpy(g["base_grad_" + name]).double()
        per_pixel = (got - ref).pow(2).sum(1).flatten()
        allowed = int(per_pixel.numel() * 1e-3)   # pixels whose nearest tap or clamp flips: at most 0.1 % may be left out
        kept = per_pixel.sort().values[:per_pixel.numel() - allowed] if allowed else per_pixel
        rel_all, rel = float(per_pixel.sum().sqrt() / ref.norm()), float(kept.sum().sqrt() / ref.norm())
        print(name, "||g - g_ref|| / ||g_ref|| =", rel_all, "without the worst", allowed, "pixels:", rel)
        assert rel <= 1e-4, name
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    from_depth, _, _, _ = _fixture_run(dev, labels_from_depth=True, with_labels=False)
    print("labels from depth", float(from_depth))
    assert abs(float(from_depth) - want) <= 2e-5 * abs(want)


def test_base_loss_does_not_synchronise(dev):
    loss, _, _, _ = _fixture_run(dev)   # (first call: the depth candidates are uploaded once and cached)
    loss.backward()
    torch.cuda.synchronize()
    inp = U.make_inputs()
    output, target = U.structure(inp, img_utils.gen_soft_label_torch, dev=dev)
    crit = get_loss(U.loss_cfg(), 0)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(output, target)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert bool(torch.isfinite(loss)) and all(v.grad is not None for v in U.volumes(output))
    # the mode is live in this build: a read-back raises under it
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            loss.item()
    finally:
        torch.cuda.set_sync_debug_mode(before)


def test_base_model_trains_with_base_loss(dev):
    from pdepth_amd.models.get_model import get_model
    cfg = synth.default_loss_cfg("default")
    torch.manual_seed(0)
    model = get_model(cfg, 0)
    synth.seed_weights(model, seed=31)
    model = model.to(dev).train()
    B, H, W = 1, 256, 384
    inputs, targets = [], []
    g = torch.Generator().manual_seed(4)
    T = torch.eye(4)
    T[0, 3] = -0.54
    for seed in (3100, 3101):
        inp = synth.make_model_input(seed, B=B, V=1, H=H, W=W, D=64, pose="mono")
        inp = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
        coarse = 8.0 + 28.0 * torch.rand(B, 1, H // 32, W // 32, generator=g)
        dmap = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        mask = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
        K_up = inp["intrinsics"].clone()
        K_up[:, :2] *= 4.0
        targets.append({"d_candi": inp["d_candi"], "T_left2right": T, "rgb": inp["rgb"], "intrinsics": inp["intrinsics"],
                        "intrinsics_up": K_up, "masks_imgsizes": mask.to(dev), "masks": mask[:, :, ::4, ::4].contiguous().to(dev),
                        "dmap_imgsizes": dmap.to(dev), "dmaps": dmap[:, ::4, ::4].contiguous().to(dev)})
        inputs.append(inp)
    crit = BaseLoss(cfg, 0, labels_from_depth=True)

    def step_loss():
        return crit(tuple(model(inputs)), tuple(targets))

    loss = step_loss()
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert bool(torch.isfinite(loss)) and len(grads) > 10 and all(bool(torch.isfinite(x).all()) for x in grads)
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    first = None
    for _ in range(4):
        opt.zero_grad()
        l = step_loss()
        first = float(l) if first is None else first
        l.backward()
        opt.step()
    last = float(step_loss())
    print("BaseModel + BaseLoss: loss", first, "->", last)
    assert last < first
