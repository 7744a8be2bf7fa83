"""GPU suite of the fused photometric term (csrc/photo.hip; ops.rgb_stereo_consistency(..., ssim_weight, ssim_md);
loss_blocks.rgb_stereo_consistency_loss(..., fused=True); BaseLoss(fused_photo=True)).

Per shape of util_photo.SHAPES and md the shape admits, at w = 0.85 with the incoming gradient 1, 2, ... per item: the mask count
equals the composition's exactly; value and every gradient element are measured against the float64 restatement of util_photo.py
next to the float32 composition's own error against it (E_ref; the composition is today's rgb_stereo_consistency_loss on the same
device: HIP warp, torch elementwise, HIP SSIM).  The rule is the project's (tests/test_loss_terms_gpu.py): a value may err by
2 E_ref + 4 ulp, a gradient element by 2 max E_ref + 1e-6 of the largest gradient.  No pixel and no window is left out.  Then:
ssim_weight = 0 is the old call, structure (repeats, NaN, empty masks, views), the loss_blocks keyword, BaseLoss, refusals."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
from pdepth_amd.utils import img_utils
import util_loss
import util_loss_terms as LT
import util_photo as P

pytestmark = pytest.mark.gpu
W = P.W_SSIM
BIG = (2, 36, 48)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- the three sides: kernel, composition (float32, same device), restatement (float64, CPU) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape, md):
    """The maker's inputs on the CPU and on the device, with the camera matrices formed on the device as BaseLoss forms them."""
    cpu = P.make_inputs(*shape, md)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in cpu.items()}
    d["Kinv"], d["proj"], _ = LT.camera_matrices(d["intr"], cpu["T"], lb._inv3)
    d["pose"] = cpu["T"].unsqueeze(0).cuda()
    for k in ("Kinv", "proj"):
        cpu[k] = d[k].cpu()
    return cpu, d


def _kernel(t, depth, w=W, md=1):
    return ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], depth, t["Kinv"], t["proj"], ssim_weight=w, ssim_md=md)[0]


def _composition(t, depth, w=W, md=1):
    return lb.rgb_stereo_consistency_loss(t["src_rgb"], t["tgt_rgb"], depth, t["pose"], t["intr"], per_item=True, ssim_weight=w, ssim_md=md)


def _function_fused(t, depth, w=W, md=1):
    return lb.rgb_stereo_consistency_loss(t["src_rgb"], t["tgt_rgb"], depth, t["pose"], t["intr"], per_item=True, ssim_weight=w, ssim_md=md,
                                          fused=True)


def _restatement(t, depth, w=W, md=1):
    return P.photo64(t["src_rgb"], t["tgt_rgb"], depth, t["Kinv"], t["proj"], w, md)[0]


def _run(fn, t, w=W, md=1, dtype=None, depth=None):
    """-> (value [B] detached, gradient of the depth) of one side, the items weighted 1, 2, ..."""
    depth = t["tgt_depth"] if depth is None else depth
    x = (depth if dtype is None else depth.to(dtype)).clone().requires_grad_(True)
    value = fn(t, x, w, md)
    (value * torch.arange(1, value.shape[0] + 1, dtype=value.dtype, device=value.device)).sum().backward()
    return value.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _reference(shape, md, w=W):
    cpu, _ = _inputs(shape, md)
    return _run(_restatement, cpu, w, md, torch.float64)


@functools.lru_cache(maxsize=None)
def _composed(shape, md, w=W):
    _, t = _inputs(shape, md)
    return _run(_composition, t, w, md)


def _mask(t):
    with torch.no_grad():
        _, valid = lb._warp(t["src_rgb"], t["tgt_depth"], t["pose"], t["intr"], "bilinear")
        return valid & lb._lower_two_thirds(valid.shape, valid.device)


def _within_the_rule(tag, got, shape, md, w=W):
    """The project's rule for (value, gradient) `got` of a float32 side against float64, E_ref from the composition."""
    (vk, gk), (vc, gc), (v64, g64) = got, _composed(shape, md, w), _reference(shape, md, w)
    vk, vc = vk.double().cpu(), vc.double().cpu()
    assert bool(torch.isfinite(v64).all()) and bool(torch.isfinite(g64).all())
    err_k, e_ref = (vk - v64).abs(), (vc - v64).abs()
    ulp = torch.from_numpy(np.spacing(v64.abs().numpy().astype(np.float32)).astype(np.float64))
    print(tag, shape, "md", md, "w", w, "value", vk.tolist(), "float64", v64.tolist(), "kernel error", err_k.tolist(), "E_ref",
          e_ref.tolist(), "ulp", ulp.tolist())
    k, c = gk.double().cpu(), gc.double().cpu()
    assert k.shape == g64.shape
    ek, er, big = float((k - g64).abs().max()), float((c - g64).abs().max()), float(g64.abs().max())
    print(tag, shape, "md", md, "w", w, "gradient: kernel max error %.3e  E_ref max %.3e  largest gradient %.3e" % (ek, er, big))
    assert bool((err_k <= 2 * e_ref + 4 * ulp).all()), (shape, md, err_k.tolist(), e_ref.tolist(), ulp.tolist())
    assert ek <= 2 * er + 1e-6 * big, (shape, md, ek, er, big)


# ---- 1, 2: count and the distance from float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,md", P.CASES)
def test_mask_count_is_the_compositions(dev, shape, md):
    _, t = _inputs(shape, md)
    value, count = ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], t["Kinv"], t["proj"], ssim_weight=W, ssim_md=md)
    want = _mask(t).reshape(shape[0], -1).sum(1).float()
    print(shape, "md", md, "count", count.tolist(), "composition", want.tolist())
    assert torch.equal(count, want) and not count.requires_grad and bool((count > 0).all())
    assert value.dtype == torch.float32 and tuple(value.shape) == (shape[0],)
    if shape == (1, 3, 3):
        assert float(count[0]) == 2.0


@pytest.mark.parametrize("shape,md", P.CASES)
def test_against_float64(dev, shape, md):
    _, t = _inputs(shape, md)
    _within_the_rule("op", _run(_kernel, t, W, md), shape, md)


# ---- 3: ssim_weight = 0 is the call it has always been -----------------------------------------------------------------------------------
def test_zero_weight_is_the_l1_pass(dev, monkeypatch):
    calls = []
    real = _native.loss_photo
    monkeypatch.setattr(_native, "loss_photo", lambda *a, **k: (calls.append("loss_photo"), real(*a, **k))[1])
    for shape in (BIG, (3, 17, 23)):
        _, t = _inputs(shape, 1)

        def plain(t, depth, w, md):
            return ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], depth, t["Kinv"], t["proj"])[0]
        v0, g0 = _run(plain, t)
        for md in (1, 3, 4):   # ignored
            v, g = _run(_kernel, t, 0.0, md)
            assert torch.equal(v, v0) and torch.equal(g, g0)
            v, g = _run(_function_fused, t, 0.0, md)   # the composition's L1 term, fused or not
            assert torch.equal(v, _run(_composition, t, 0.0, md)[0])
        outside = ~_mask(t)
        assert int(outside.sum()) > 0 and bool((g0[outside] == 0).all())
        with torch.no_grad():
            assert torch.equal(_kernel(t, t["tgt_depth"], 0, 1), v0)
    assert calls == []


# ---- 4: structure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md", (1, 2, 3))
def test_repeats_carry_the_same_bits(dev, md):
    _, t = _inputs((2, 33, 66), md)
    (v1, g1), (v2, g2) = _run(_kernel, t, W, md), _run(_kernel, t, W, md)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    with torch.no_grad():
        assert torch.equal(_kernel(t, t["tgt_depth"], W, md), v1)


@pytest.mark.parametrize("md", (1, 3))
def test_nan_depth_stays_in_its_item(dev, md):
    _, t = _inputs(BIG, md)
    clean_v, clean_g = _run(_kernel, t, W, md)
    for row in (20, 2):   # inside the mask; behind a zero mask (the top third): NaN * 0 is still NaN
        depth = t["tgt_depth"].clone()
        depth[0, row, 10] = float("nan")
        v, g = _run(_kernel, t, W, md, depth=depth)
        want = _composition(t, depth, W, md)
        print("md", md, "row", row, "value", v.tolist(), "composition", want.tolist())
        assert bool(torch.isnan(v[0])) and bool(torch.isnan(want[0]))
        assert torch.equal(v[1], clean_v[1]) and torch.equal(g[1], clean_g[1]) and bool(torch.isfinite(g[1]).all())


def test_empty_mask_is_nan_for_its_item_alone(dev):
    _, t = _inputs(BIG, 1)
    clean_v, clean_g = _run(_kernel, t)
    depth = t["tgt_depth"].clone()
    depth[1] = 0.01   # so near that every sample lands outside the source
    value, count = ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], depth, t["Kinv"], t["proj"], ssim_weight=W)
    want = _composition(t, depth)
    print("value", value.tolist(), "count", count.tolist(), "composition", want.tolist())
    assert float(count[1]) == 0.0 and bool(torch.isnan(value[1])) and bool(torch.isnan(want[1]))
    assert torch.equal(value[0], clean_v[0])
    v, g = _run(_kernel, t, depth=depth)
    assert torch.equal(g[0], clean_g[0])


def test_view_gives_the_bits_of_its_copy(dev):
    _, t = _inputs((2, 18, 129), 2)
    v0, g0 = _run(_kernel, t, W, 2)
    wide = torch.zeros(2, 18, 258, device=dev)
    wide[:, :, ::2] = t["tgt_depth"]
    wide.requires_grad_(True)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    value = _kernel(t, view, W, 2)
    (value * torch.arange(1, 3, dtype=value.dtype, device=dev)).sum().backward()
    assert torch.equal(value.detach(), v0) and torch.equal(wide.grad[:, :, ::2], g0) and not bool(wide.grad[:, :, 1::2].any())
    col = ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"].unsqueeze(1), t["Kinv"], t["proj"], ssim_weight=W, ssim_md=2)[0]
    assert torch.equal(col, v0)   # [B,1,H,W], the reference's layout of a depth map


# ---- 5: the keyword of loss_blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", (1.0, 0.85))
def test_function_fused_against_the_composition(dev, w):
    _, t = _inputs(BIG, 1)
    got = _run(_function_fused, t, w, 1)
    _within_the_rule("loss_blocks fused", got, BIG, 1, w)
    one = {k: (v[:1] if isinstance(v, torch.Tensor) and v.dim() >= 3 and v.shape[0] == 2 else v) for k, v in t.items()}
    with torch.no_grad():
        scalar = lb.rgb_stereo_consistency_loss(one["src_rgb"], one["tgt_rgb"], one["tgt_depth"], one["pose"], one["intr"], ssim_weight=w,
                                                fused=True)
    assert scalar.dim() == 0 and torch.equal(scalar, got[0][0])


# ---- 6: BaseLoss ---------------------------------------------------------------------------------------------------------------------------
ONLY_RSC = dict(ce_mul=0.0, dsc_mul=0.0, dc_mul=0.0, smooth_mul=0.0, rsc_low_mul=0.0, rsc_mul=1.0)


def _cfg(**loss):
    cfg = util_loss.loss_cfg()
    cfg.loss.__dict__.update(loss)
    return cfg


def _base_run(dev, cfg, **switches):
    output, target = util_loss.structure(util_loss.make_inputs(), img_utils.gen_soft_label_torch, dev=dev)
    loss = BaseLoss(cfg, 0, **switches)(output, target)
    loss.backward()
    return loss.detach(), [v.grad for v in util_loss.volumes(output)], (output, target)


def _share(dev, output, target, low):
    """The sum over the two directions of the op's per-item values, on the depth maps BaseLoss regresses (ops.dpv_soft_ce)."""
    tl, tr = target
    B = util_loss.B
    with torch.no_grad():
        depth = {}
        for s, out, tg in (("l", output[0], tl), ("r", output[1], tr)):
            vol, mk, lab = (out["output"][0], "masks", "soft_labels") if low else (out["output_refined"][0], "masks_imgsizes", "soft_labels_imgsize")
            depth[s] = ops.dpv_soft_ce(vol, tl["d_candi"], mask=tg[mk][:, 0], want_depth=True, label=torch.stack(list(tg[lab])))[1]
        T = tl["T_left2right"].float()
        pose = {"l": T.unsqueeze(0).to(dev), "r": torch.inverse(T).unsqueeze(0).to(dev)}
        rgb = {"l": tl["rgb"][:, -1], "r": tr["rgb"][:, -1]}
        if low:
            rgb = {s: torch.nn.functional.interpolate(v, scale_factor=0.25, mode="bilinear") for s, v in rgb.items()}
        total = 0
        for s, o, tg in (("l", "r", tl), ("r", "l", tr)):   # the target side, the source side
            k = tg["intrinsics" if low else "intrinsics_up"].float()
            Kinv, proj = lb._inv3(k).expand(B, 3, 3), torch.matmul(k, pose[s][:, 0:3, :]).expand(B, 3, 4)
            total = total + ops.rgb_stereo_consistency(rgb[o], rgb[s], depth[s], Kinv, proj, ssim_weight=W)[0].sum()
        return total


def test_base_loss_fused_photo(dev, monkeypatch):
    calls = []
    for name in ("loss_photo", "ssim", "loss_rsc"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    bsize = float(2 * util_loss.B)
    for low, n_calls in ((False, 2), (True, 4)):
        del calls[:]
        cfg = _cfg(rsc_ssim=W, **dict(ONLY_RSC, rsc_low_mul=1.0 if low else 0.0))
        loss, grads, (output, target) = _base_run(dev, cfg, fused_terms=True, fused_photo=True)
        assert calls == ["loss_photo"] * n_calls, calls
        for g in (grads[1], grads[3]):   # the refined volumes of the left and the right side
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        del calls[:]
        want = _share(dev, output, target, False) / bsize
        if low:
            assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in (grads[0], grads[2]))
            want = want + _share(dev, output, target, True) / bsize
        composed, _, _ = _base_run(dev, cfg, fused_terms=True)
        print("BaseLoss(fused_photo=True) low", low, float(loss), "the op's values", float(want), "composition", float(composed))
        assert torch.equal(loss, want)
        assert abs(float(loss) - float(composed)) <= 1e-5 * abs(float(composed))
        # without fused_terms the switch still selects the op
        alone, _, _ = _base_run(dev, cfg, fused_photo=True)
        assert torch.equal(alone, loss)


def test_base_loss_without_the_key_ignores_the_switch(dev, monkeypatch):
    """rsc_ssim absent (or 0): fused_photo=True gives the bits of fused_photo=False, on both paths of the other terms (dsc off: its
    source gradient is summed with float atomics, whose last bits differ from run to run)."""
    calls = []
    real = _native.loss_photo
    monkeypatch.setattr(_native, "loss_photo", lambda *a, **k: (calls.append("loss_photo"), real(*a, **k))[1])
    for extra in ({}, {"rsc_ssim": 0.0, "rsc_ssim_md": 2}):
        for fused in (False, True):
            off = _base_run(dev, _cfg(dsc_mul=0.0, rsc_low_mul=1.0, **extra), fused_terms=fused)
            on = _base_run(dev, _cfg(dsc_mul=0.0, rsc_low_mul=1.0, **extra), fused_terms=fused, fused_photo=True)
            assert torch.equal(off[0], on[0]) and all(torch.equal(a, b) for a, b in zip(off[1], on[1]))
    assert calls == []


# ---- 7: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(dev):
    _, t = _inputs((1, 7, 7), 1)
    args = (t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], t["Kinv"], t["proj"])
    with pytest.raises(NotImplementedError, match="md=4"):
        ops.rgb_stereo_consistency(*args, ssim_weight=W, ssim_md=4)
    wide = torch.rand(1, 3, 2, 9, device=dev)
    with pytest.raises(RuntimeError, match="H=2, W=9"):
        ops.rgb_stereo_consistency(wide, wide, torch.ones(1, 2, 9, device=dev), t["Kinv"], t["proj"], ssim_weight=W)
    with pytest.raises(RuntimeError, match=r"src_rgb must be \[1, 3, 7, 7\]"):
        ops.rgb_stereo_consistency(wide, *args[1:], ssim_weight=W)
    with pytest.raises(RuntimeError, match=r"proj must be \[1, 3, 4\]"):
        ops.rgb_stereo_consistency(*args[:4], t["proj"][:, :, :3], ssim_weight=W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgb_stereo_consistency(args[0].cpu(), *args[1:], ssim_weight=W)
    for name in ("src_rgb", "tgt_rgb", "Kinv", "proj"):
        named = dict(zip(("src_rgb", "tgt_rgb", "tgt_depth", "Kinv", "proj"), args))
        named[name] = named[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=f"rgb_stereo_consistency: {name} requires grad"):
            ops.rgb_stereo_consistency(*named.values(), ssim_weight=W)
    x = t["tgt_depth"].clone().requires_grad_(True)   # once_differentiable: a second-order gradient raises, it is not a constant
    (g,) = torch.autograd.grad(ops.rgb_stereo_consistency(*args[:2], x, *args[3:], ssim_weight=W)[0].sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # the C entries, past the binding's own checks
    lib = _native.load()
    out = torch.empty(2, 1, device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    ptrs = [a.contiguous().data_ptr() for a in args]
    tail = (out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), 256, None)
    assert lib.pdepth_loss_photo_f32(*ptrs, 1, 7, 7, W, 4, *tail) == 1 and b"md=4" in lib.pdepth_last_error()
    assert lib.pdepth_loss_photo_f32(*ptrs, 1, 2, 9, W, 1, *tail) == 1 and b"H=2, W=9" in lib.pdepth_last_error()
    assert lib.pdepth_loss_photo_f32(*ptrs, 1, 7, 7, W, 1, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), 255, None) == 3
    g = torch.empty(1, 7, 7, device=dev)
    back = (out[1].data_ptr(), out[0].data_ptr(), 1, 7, 7, W)
    assert lib.pdepth_loss_photo_backward_f32(*ptrs, *back, 4, g.data_ptr(), None) == 1 and b"md=4" in lib.pdepth_last_error()
    assert lib.pdepth_loss_photo_backward_f32(*ptrs, *back, 1, None, None) == 1 and b"null pointer" in lib.pdepth_last_error()
