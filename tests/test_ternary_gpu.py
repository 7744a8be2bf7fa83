"""GPU suite of the ternary census op (csrc/ternary.hip), forward and backward, against the float64 restatement of
tests/util_ternary.py.

The bound is the reference's own, as in tests/test_ssim_gpu.py: E_ref = the distance of the reference's float32 result (fixture
g26_ternary; beyond the fixture: the float32 torch composition of the same formula) from the float64 restatement, and the kernel may
be at
    forward   2 E_ref + 2^-23                 (one ulp at the output's scale, 1)
    backward  2 E_ref_grad + 2^-23 max |g64|  (one ulp of the largest gradient)
from it: kernel and reference are two float32 evaluations with different summation orders, and the ulp term covers the cases whose
E_ref is 0.  The function is smooth: every pixel of every case counts.  Then the output selection, the reproducibility, the
autograd binding, and the losses that mix the op in."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops, synth
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
from pdepth_amd.utils import img_utils
import util_loss
import util_loss_terms as LT
import util_ternary as U

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
NAMES = [f"{kind}_md{md}" for md in U.MDS for kind in U.KINDS]
TILE_W, TILE_H = U.tile()   # csrc/ternary.hip: TERN_TW, TERN_TH


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- references, computed once -------------------------------------------------------------------------------------------------------
def _reference(x, y, g, md, ref_dist, ref_gx, ref_gy):
    """float64 results of a case and the float32 reference's distance from them."""
    x64, y64, g64 = (torch.from_numpy(np.ascontiguousarray(a)).double() for a in (x, y, g))
    dist = U.ternary_dist(x64, y64, md)
    gx, gy = U.ternary_grads(x64, y64, g64, md)
    return {"dist": dist, "g": (gx, gy), "E": float((torch.from_numpy(ref_dist).double() - dist).abs().max()),
            "E_g": (float((torch.from_numpy(ref_gx).double() - gx).abs().max()), float((torch.from_numpy(ref_gy).double() - gy).abs().max()))}


@functools.lru_cache(maxsize=None)
def _fixture_reference(name):
    c = U.cases()[name]
    return _reference(c["x"], c["y"], c["g_out"], c["md"], c["dist"], c["g_x"], c["g_y"])


def _composition32(x, y, g, md):
    """The float32 torch composition of the formula on the CPU, forward and autograd: what stands in for the fixture beyond it."""
    tx, ty, tg = (torch.from_numpy(a) for a in (x, y, g))
    gx, gy = U.ternary_grads(tx, ty, tg, md)
    return U.ternary_dist(tx, ty, md).numpy(), gx.numpy(), gy.numpy()


# shapes beyond the fixture: one row of interior pixels across a tile edge; W - 2 md = the tile width and one either side of it, H
# spanning two rows of tiles; whole tiles exactly; a non-contiguous view
EXTRA = [(md, kind) for md in U.MDS for kind in ("row", "w-1", "w", "w+1", "tiles", "view")]


@functools.lru_cache(maxsize=None)
def _extra(md, kind):
    two_rows = TILE_H + 3
    shape = {"row": (1, 3, 2 * md + 1, TILE_W + 6), "w-1": (2, 3, two_rows, TILE_W + 2 * md - 1), "w": (2, 3, two_rows, TILE_W + 2 * md),
             "w+1": (2, 3, two_rows, TILE_W + 2 * md + 1), "tiles": (1, 3, 2 * TILE_H, TILE_W), "view": (2, 3, 13, 33)}[kind]
    rng = np.random.RandomState(7600 + 10 * md + len(kind))
    B, C, H, W = shape
    big = (B, C, 2 * H, W + 2) if kind == "view" else shape
    x = rng.uniform(0, 1, big).astype(np.float32)
    y = np.clip(x + np.float32(0.1) * rng.standard_normal(big).astype(np.float32), 0, 1).astype(np.float32)
    g = rng.standard_normal((B, 1, H, W)).astype(np.float32)
    sel = (lambda a: a[:, :, ::2, 1:-1]) if kind == "view" else (lambda a: a)
    xs, ys = np.ascontiguousarray(sel(x)), np.ascontiguousarray(sel(y))
    return (x, y, g, sel), _reference(xs, ys, g, md, *_composition32(xs, ys, g, md))


def _check_forward(tag, got, ref):
    err = float((got.double().cpu() - ref["dist"]).abs().max())
    print(tag, "forward max |kernel - f64| = %.3e  E_ref = %.3e  bound %.3e" % (err, ref["E"], 2 * ref["E"] + ULP))
    assert err <= 2 * ref["E"] + ULP, tag


def _check_backward(tag, got, ref):
    for i, side in enumerate(("g_x", "g_y")):
        err = float((got[i].double().cpu() - ref["g"][i]).abs().max())
        big = float(ref["g"][i].abs().max())
        bound = 2 * ref["E_g"][i] + ULP * big
        print(tag, side, "max |kernel - f64| = %.3e  E_ref_grad = %.3e  max |g64| = %.3e  bound %.3e" % (err, ref["E_g"][i], big, bound))
        assert err <= bound, (tag, side)


# ---- the kernels against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_fixture(dev, name):
    c = U.cases()[name]
    got = ops.ternary(torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["y"]).to(dev), c["md"])
    assert got.dtype == torch.float32 and tuple(got.shape) == c["dist"].shape
    _check_forward(name, got, _fixture_reference(name))
    if name.startswith(("same", "const")):   # identical inputs are at distance 0 exactly
        assert int(torch.count_nonzero(got)) == 0


@pytest.mark.parametrize("name", NAMES)
def test_backward_fixture(dev, name):
    c = U.cases()[name]
    x, y, g = (torch.from_numpy(c[k]).to(dev) for k in ("x", "y", "g_out"))
    x.requires_grad_(True), y.requires_grad_(True)
    (ops.ternary(x, y, c["md"]) * g).sum().backward()
    assert x.grad.shape == x.shape and y.grad.shape == y.shape
    _check_backward(name, (x.grad, y.grad), _fixture_reference(name))
    if name.startswith(("same", "const")):
        assert int(torch.count_nonzero(x.grad)) == 0 and int(torch.count_nonzero(y.grad)) == 0


@pytest.mark.parametrize("md,kind", EXTRA)
def test_shapes_beyond_the_fixture(dev, md, kind):
    (x, y, g, sel), ref = _extra(md, kind)
    tx, ty = sel(torch.from_numpy(x).to(dev)), sel(torch.from_numpy(y).to(dev))
    assert tx.is_contiguous() == (kind != "view")
    tag = f"md{md} {kind} {list(tx.shape)}"
    _check_forward(tag, ops.ternary(tx, ty, md), ref)
    gx, gy = _native.ternary_backward(tx, ty, torch.from_numpy(g).to(dev), md)
    _check_backward(tag, (gx, gy), ref)


# ---- output selection, reproducibility, the autograd binding --------------------------------------------------------------------------
@pytest.mark.parametrize("md", U.MDS)
def test_one_gradient_is_the_two_gradient_call(dev, md):
    c = U.cases()[f"masked_md{md}"]
    x, y, g = (torch.from_numpy(c[k]).to(dev) for k in ("x", "y", "g_out"))
    assert torch.equal(ops.ternary(x, y, md), ops.ternary(x, y, md))
    gx, gy = _native.ternary_backward(x, y, g, md)
    again = _native.ternary_backward(x, y, g, md)
    assert torch.equal(gx, again[0]) and torch.equal(gy, again[1])
    only_x = _native.ternary_backward(x, y, g, md, want_y=False)
    only_y = _native.ternary_backward(x, y, g, md, want_x=False)
    assert only_x[1] is None and only_y[0] is None
    assert torch.equal(only_x[0], gx) and torch.equal(only_y[1], gy)


def test_autograd_asks_for_the_needed_gradients_only(dev, monkeypatch):
    c = U.cases()["noisy_md1"]
    x, y, g = (torch.from_numpy(c[k]).to(dev) for k in ("x", "y", "g_out"))
    plain = ops.ternary(x, y, 1)
    asked = []
    real = _native.ternary_backward
    monkeypatch.setattr(_native, "ternary_backward", lambda *a, **k: (asked.append((k["want_x"], k["want_y"])), real(*a, **k))[1])
    both = _native.ternary_backward(x, y, g, 1, want_x=True, want_y=True)
    for wx, wy in ((True, False), (False, True), (True, True)):
        a, b = x.clone().requires_grad_(wx), y.clone().requires_grad_(wy)
        out = ops.ternary(a, b, 1)
        assert torch.equal(out, plain)   # the forward under autograd is the no-grad kernel call
        (out * g).sum().backward()
        assert asked[-1] == (wx, wy)
        assert (a.grad is not None) == wx and (b.grad is not None) == wy
        if wx:
            assert torch.equal(a.grad, both[0])
        if wy:
            assert torch.equal(b.grad, both[1])
    assert torch.equal(lb.TernaryLoss(x, y), plain) and torch.equal(lb.TernaryLoss(x, y, max_distance=1), plain)
    assert torch.equal(lb.TernaryLoss(x, y, 2), ops.ternary(x, y, 2)) and not torch.equal(ops.ternary(x, y, 2), plain)


def test_refusals_on_the_device(dev):
    x = torch.rand(1, 3, 9, 9, device=dev)
    with pytest.raises(RuntimeError, match=r"g_out must be \[1, 1, 9, 9\]"):
        _native.ternary_backward(x, x, torch.zeros(1, 1, 7, 7, device=dev), 1)
    with pytest.raises(RuntimeError, match="no gradient requested"):
        _native.ternary_backward(x, x, torch.zeros(1, 1, 9, 9, device=dev), 1, want_x=False, want_y=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ternary(x, x.cpu())
    lib = _native.load()   # the C entry's own words, past the binding's checks
    s = _native._stream(dev)
    out = torch.empty(1, 1, 9, 9, device=dev)
    assert lib.pdepth_ternary_f32(x.data_ptr(), x.data_ptr(), 1, 9, 9, 4, out.data_ptr(), s) == 1
    assert b"md=4" in lib.pdepth_last_error()
    assert lib.pdepth_ternary_f32(x.data_ptr(), x.data_ptr(), 1, 2, 9, 1, out.data_ptr(), s) == 1
    assert b"H=2, W=9" in lib.pdepth_last_error()


# ---- the loss -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stereo_pair():
    """The [2,3,24,40] stereo pair of tests/test_ssim_gpu.py, rebuilt: images in [0,1] that share their coarse structure, a smooth
    depth map, synth's stereo pose."""
    B, H, W = 2, 24, 40
    rng = np.random.RandomState(8500)
    R, t = synth.make_pose("stereo", rng)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    coarse = torch.from_numpy(rng.uniform(0, 1, (B, 3, H // 4, W // 4)))
    base = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    src = (0.8 * base + 0.2 * torch.from_numpy(rng.uniform(0, 1, (B, 3, H, W)))).float()
    tgt = (0.8 * base + 0.2 * torch.from_numpy(rng.uniform(0, 1, (B, 3, H, W)))).float()
    depth = LT._smooth_depth(rng, B, H, W).float()
    return src, tgt, depth, torch.from_numpy(T).float().unsqueeze(0), LT.intrinsics(B, H, W)


def _photo(dev, monkeypatch, census, **kw):
    """rgb_stereo_consistency_loss per item on the pair, TernaryLoss replaced by `census` (None: the op) -> (value [B], depth
    gradient)."""
    src, tgt, depth, pose, intr = (t.to(dev) for t in _stereo_pair())
    depth = depth.clone().requires_grad_(True)
    if census is not None:
        monkeypatch.setattr(lb, "TernaryLoss", census)
    value = lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, **kw)
    monkeypatch.undo()
    if depth.requires_grad and value.requires_grad:
        value.sum().backward()
    return value.detach(), depth.grad


def test_loss_without_the_census_term_keeps_its_bits(dev, monkeypatch):
    called = []
    real = _native.ternary
    for ssim in ({}, {"ssim_weight": 0.85, "ssim_md": 2}):
        plain, g_plain = _photo(dev, monkeypatch, None, **ssim)
        monkeypatch.setattr(_native, "ternary", lambda *a, **k: (called.append(1), real(*a, **k))[1])
        zero, g_zero = _photo(dev, monkeypatch, None, ternary_weight=0.0, ternary_md=2, **ssim)
        assert called == []   # the op is not called
        assert torch.equal(plain, zero) and torch.equal(g_plain, g_zero)
    src, tgt, depth, pose, intr = (t.to(dev) for t in _stereo_pair())
    assert torch.equal(lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr),
                       lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, ternary_weight=0.0))


@pytest.mark.parametrize("md", (1, 2))
@pytest.mark.parametrize("ws,wt", ((0.0, 0.5), (0.425, 0.425)))
def test_loss_with_the_census_term_against_the_composition(dev, monkeypatch, ws, wt, md):
    """The value and the depth gradient of the function with the HIP op against the same function whose TernaryLoss is
    util_ternary's torch composition in float32 on the device, to within twice that composition's own distance from its float64
    form (the same function, the census term composed in float64) on these inputs."""
    kw = {"ssim_weight": ws, "ternary_weight": wt, "ternary_md": md}
    calls = []
    real = _native.ssim
    monkeypatch.setattr(_native, "ssim", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    v_k, g_k = _photo(dev, monkeypatch, None, **kw)
    assert len(calls) == (0 if ws == 0 else 1)   # a piece whose weight is 0 is not evaluated
    v_c, g_c = _photo(dev, monkeypatch, lambda x, y, m=1: U.ternary_dist(x, y, m), **kw)
    v_64, g_64 = _photo(dev, monkeypatch, lambda x, y, m=1: U.ternary_dist(x.double(), y.double(), m), **kw)
    l1, _ = _photo(dev, monkeypatch, None, ssim_weight=ws)
    assert bool(torch.isfinite(v_k).all()) and bool(torch.isfinite(g_k).all()) and not torch.equal(v_k, l1)
    dv, ev = float((v_k.double() - v_c.double()).abs().max()), float((v_c.double() - v_64.double()).abs().max())
    dg, eg = float((g_k.double() - g_c.double()).abs().max()), float((g_c.double() - g_64.double()).abs().max())
    print("ws", ws, "wt", wt, "md", md, "value", v_k.tolist(), "|kernel - composition| = %.3e  composition's |f32 - f64| = %.3e" % (dv, ev))
    print("ws", ws, "wt", wt, "md", md, "max |g| = %.3e  |kernel - composition| = %.3e  composition's |f32 - f64| = %.3e"
          % (float(g_64.abs().max()), dg, eg))
    assert dv <= 2 * ev
    assert dg <= 2 * eg


def test_loss_refuses_fused_with_a_census_term(dev):
    src, tgt, depth, pose, intr = (t.to(dev) for t in _stereo_pair())
    for ws in (0.0, 0.425):
        with pytest.raises(RuntimeError, match="no census term"):
            lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, fused=True, ssim_weight=ws, ternary_weight=0.425)


# ---- BaseLoss -------------------------------------------------------------------------------------------------------------------------
def _base_cfg(**loss):
    cfg = util_loss.loss_cfg()
    cfg.loss.__dict__.update(loss)
    return cfg


def _base_run(dev, cfg, **how):
    output, target = util_loss.structure(util_loss.make_inputs(), img_utils.gen_soft_label_torch, dev=dev)
    loss = BaseLoss(cfg, 0, **how)(output, target)
    loss.backward()
    return loss.detach(), [v.grad for v in util_loss.volumes(output)], (output, target)


def test_base_loss_without_the_key_keeps_its_bits(dev):
    """rsc_ternary absent = rsc_ternary 0, bit for bit, on both settings of fused_terms (dsc off: its source gradient is summed with
    float atomics, whose last bits differ from run to run with or without this change)."""
    for fused in (False, True):
        absent = _base_run(dev, _base_cfg(dsc_mul=0.0, rsc_low_mul=1.0), fused_terms=fused)
        zero = _base_run(dev, _base_cfg(dsc_mul=0.0, rsc_low_mul=1.0, rsc_ternary=0.0, rsc_ternary_md=2), fused_terms=fused)
        assert torch.equal(absent[0], zero[0])
        assert all(torch.equal(a, b) for a, b in zip(absent[1], zero[1]))


def test_base_loss_with_the_census_term(dev, monkeypatch):
    """With rsc_ternary = 0.5 and only rsc_mul on: both sides' refined volumes get finite non-zero gradients, the loss is the two
    rgb_stereo_consistency_loss(..., ternary_weight=0.5) calls summed over 2 B, and fused_terms and fused_photo give that same
    loss: the rsc term is the composition around the HIP op whatever they say."""
    only_rsc = dict(ce_mul=0.0, dsc_mul=0.0, dc_mul=0.0, smooth_mul=0.0, rsc_low_mul=0.0, rsc_mul=1.0)
    calls = []
    for name in ("loss_rsc", "loss_photo", "ssim", "ternary"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    loss, grads, (output, target) = _base_run(dev, _base_cfg(rsc_ternary=0.5, **only_rsc))
    assert calls == ["ternary", "ternary"]
    hi = [grads[1], grads[3]]   # the refined volumes of the left and the right side: the depth maps the rsc term warps with
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in hi)
    plain, _, _ = _base_run(dev, _base_cfg(**only_rsc))
    assert not torch.equal(plain, loss)
    # the share, from the depth maps BaseLoss regresses (ops.dpv_soft_ce) and the function itself
    tl, tr = target
    dc = tl["d_candi"]
    depth = {}
    with torch.no_grad():
        for s, out, tg in (("l", output[0], tl), ("r", output[1], tr)):
            depth[s] = ops.dpv_soft_ce(out["output_refined"][0], dc, mask=tg["masks_imgsizes"][:, 0], want_depth=True,
                                       label=torch.stack(list(tg["soft_labels_imgsize"])))[1]
        T = tl["T_left2right"].float()
        l2r, r2l = T.unsqueeze(0).to(dev), torch.inverse(T).unsqueeze(0).to(dev)
        rgb_l, rgb_r = tl["rgb"][:, -1], tr["rgb"][:, -1]
        want = (lb.rgb_stereo_consistency_loss(rgb_r, rgb_l, depth["l"], l2r, tl["intrinsics_up"], per_item=True, ternary_weight=0.5).sum() +
                lb.rgb_stereo_consistency_loss(rgb_l, rgb_r, depth["r"], r2l, tr["intrinsics_up"], per_item=True, ternary_weight=0.5).sum())
        want = want / (2 * util_loss.B)
    print("BaseLoss rsc share with the census term", float(loss), "the function", float(want), "without it", float(plain))
    assert torch.equal(loss, want)
    for how in ({"fused_terms": True}, {"fused_photo": True}, {"fused_terms": True, "fused_photo": True}):
        del calls[:]
        again, g_again, _ = _base_run(dev, _base_cfg(rsc_ternary=0.5, **only_rsc), **how)
        assert calls == ["ternary", "ternary"], (how, calls)
        assert torch.equal(again, loss), how
        assert all(torch.equal(a, b) for a, b in zip(g_again[1::2], hi)), how
    # with the SSIM beside it, md = 2 and the low-resolution term on: the three-piece mix, the same on every setting
    mix = dict(only_rsc, rsc_low_mul=1.0, rsc_ssim=0.425, rsc_ternary=0.425, rsc_ternary_md=2)
    del calls[:]
    three, g_three, _ = _base_run(dev, _base_cfg(**mix))
    assert sorted(calls) == ["ssim"] * 4 + ["ternary"] * 4 and bool(torch.isfinite(three)) and not torch.equal(three, loss)
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in g_three)
    assert torch.equal(_base_run(dev, _base_cfg(**mix), fused_terms=True, fused_photo=True)[0], three)
