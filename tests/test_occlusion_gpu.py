"""GPU suite of the range map and the occlusion masks (csrc/occlusion.hip) against the float64 restatement of
tests/util_occlusion.py and the fixture g27_occlusion.

The contract (include/pdepth.h):
  positions  |r - r64(the same float32 positions)| <= 2^-22 (1 + contributions of the destination): each weight is two fp32
             roundings of numbers <= 1, the integer sum is exact up to the final rounding; exact where the weights are dyadic;
  depth      |r - r64| <= 4 e32, e32 = the float32 reference's own distance from its float64 run on the case (fixture): the kernel
             associates the 3x3 and 3x4 products differently from ATen's bmm, both chains of a few ulp;
  masks      equal to the float64 mask at every pixel: no pixel of a case lies within 1e-3 of a threshold (the fixture maker's
             condition on the inputs), so this is a plain equality;
  bits       the same from call to call, on another stream and with the batch reversed.
Then the loss functions and BaseLoss with the masks."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
from pdepth_amd.utils import img_utils
from pdepth_amd.utils import inverse_warp as iv
from pdepth_amd.utils import warp_utils as wu
import util_loss
import util_occlusion as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _key(th):
    return str(th).replace("0.", "")


# ---- references, computed once on the CPU -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flow_reference(name):
    pos = U.base_grid(2, 16, 16) + torch.from_numpy(U.cases()[name]["flow"])
    return pos, U.range_map(pos.double())


@functools.lru_cache(maxsize=None)
def _position_reference(name):
    """Of a depth case: the reference's float32 positions, the float64 range map of exactly those, the contributions."""
    pos = torch.from_numpy(U.cases()[name]["pos32"])
    r64, n = U.range_map(pos.double(), want_count=True)
    return pos, r64, n


def _depth_inputs(name, dev):
    c = U.cases()[name]
    return tuple(torch.from_numpy(c[k]).to(dev) for k in ("depth", "Kinv", "proj"))


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FLOW_CASES)
def test_dyadic_weights_are_exact(dev, name):
    """Integer and quarter-pixel flows, the 256-fold collision, positions on and one beyond the last row and column, and non-finite
    positions (which add nothing): the range map is the restatement's, bit for bit, and so are both masks."""
    pos, r64 = _flow_reference(name)
    r = ops.range_map(pos.to(dev))
    assert r.dtype == torch.float32 and tuple(r.shape) == (2, 1, 16, 16)
    assert torch.equal(r.cpu().double(), r64)
    assert torch.equal(wu.get_corresponding_map(pos.to(dev)), r)
    for th in U.THS:
        vis, again = ops.occlusion_mask(pos.to(dev), th=th, want_range=True)
        assert torch.equal(again, r) and torch.equal(vis.cpu(), U.visible(r64, th))
        assert torch.equal(ops.occlusion_mask(pos.to(dev), th), vis)
    if name == "e_collide":
        x, y = U.COLLIDE_AT
        assert float(r[0, 0, y, x]) == 256.0 and float(r[1].sum()) == 256.0


def test_mask_of_the_two_disparity_flow_is_the_analytic_band(dev):
    flow = torch.from_numpy(U.cases()["e_int"]["flow"]).to(dev)
    occ = wu.get_occu_mask_backward(flow)
    assert occ.dtype == torch.float32 and tuple(occ.shape) == (2, 1, 16, 16)
    assert np.array_equal(1 - occ[0, 0].cpu().numpy(), U.analytic_band())
    c = U.cases()["e_int"]
    for th in U.THS:
        assert np.array_equal(wu.get_occu_mask_backward(flow, th=th).cpu().numpy(), c[f"occ32_{_key(th)}"].astype(np.float32))


# ---- the two entries on the scenes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.DEPTH_CASES)
def test_position_entry_on_the_scenes(dev, name):
    pos, r64, n = _position_reference(name)
    r = ops.range_map(pos.to(dev)).cpu().double()
    err, bound = (r - r64).abs(), 2.0 ** -22 * (1 + n)
    print(name, "positions: max |r - r64| = %.3e, the bound there %.3e, max contributions %d"
          % (float(err.max()), float(bound.flatten()[err.argmax()]), int(n.max())))
    assert bool((err <= bound).all())
    c = U.cases()[name]
    for th in U.THS:
        vis = ops.occlusion_mask(pos.to(dev), th=th)
        assert torch.equal(vis.cpu(), U.visible(r64, th))
        assert np.array_equal(1 - vis.cpu().numpy(), c[f"occ64_{_key(th)}"].astype(np.float32))


@pytest.mark.parametrize("name", U.DEPTH_CASES)
def test_depth_entry_on_the_scenes(dev, name):
    c = U.cases()[name]
    depth, Kinv, proj = _depth_inputs(name, dev)
    r64, e32 = torch.from_numpy(c["r64"]), float(c["e32"])
    for th in U.THS:
        vis, r = ops.depth_occlusion(depth, Kinv, proj, th=th, want_range=True)
        err = float((r.cpu().double() - r64).abs().max())
        print(name, "depth: max |r - r64| = %.3e, e32 = %.3e" % (err, e32))
        assert err <= 4 * e32
        assert np.array_equal(1 - vis.cpu().numpy(), c[f"occ64_{_key(th)}"].astype(np.float32))
        assert torch.equal(ops.depth_occlusion(depth[:, None], Kinv, proj, th), vis)
    # a depth map that requires grad is accepted; the mask is a constant
    leaf = depth.clone().requires_grad_(True)
    got = ops.depth_occlusion(leaf * 1.0, Kinv, proj, th=0.5, want_range=True)
    assert all(t.grad_fn is None and not t.requires_grad for t in got) and torch.equal(got[0], vis) and torch.equal(got[1], r)


def test_src_mask_is_honoured(dev):
    """Case c: the holes as depth 0 and as src_mask 0 on the map without holes.  A masked pixel adds nothing: the restatement with
    those positions made NaN.  (A depth of 0 lands far outside -- Z is clamped to 1e-3 -- so both give the same map here.)"""
    c = U.cases()["c"]
    depth, Kinv, proj = _depth_inputs("c", dev)
    full = torch.from_numpy(c["depth_full"]).to(dev)
    keep = torch.from_numpy(1.0 - c["holes"].astype(np.float32)).to(dev)
    pos = U.depth_positions(*(torch.from_numpy(c[k]).double() for k in ("depth_full", "Kinv", "proj")))
    pos = torch.where(torch.from_numpy(c["holes"]).bool().unsqueeze(1), torch.full_like(pos, float("nan")), pos)
    r64 = U.range_map(pos)
    assert float((r64 - torch.from_numpy(c["r64"])).abs().max()) <= 1e-12
    vis, r = ops.depth_occlusion(full, Kinv, proj, src_mask=keep, want_range=True)
    assert float((r.cpu().double() - r64).abs().max()) <= 4 * float(c["e32"])
    assert torch.equal(vis.cpu(), U.visible(r64, 0.2))
    assert torch.equal(ops.depth_occlusion(full[:, None], Kinv, proj, src_mask=keep[:, None]), vis)
    unmasked = ops.depth_occlusion(full, Kinv, proj, want_range=True)[1]
    assert not torch.equal(unmasked, r) and float(unmasked.sum()) > float(r.sum())
    nothing = ops.depth_occlusion(full, Kinv, proj, src_mask=torch.zeros_like(keep), want_range=True)
    assert int(torch.count_nonzero(nothing[0])) == 0 and int(torch.count_nonzero(nothing[1])) == 0


def test_bits_do_not_depend_on_the_run_the_stream_or_the_neighbours(dev):
    pos = torch.from_numpy(U.cases()["b"]["pos32"]).to(dev)
    depth, Kinv, proj = _depth_inputs("b", dev)
    calls = (lambda p, d, k, m: ops.occlusion_mask(p, 0.2, want_range=True), lambda p, d, k, m: ops.depth_occlusion(d, k, m, 0.2, want_range=True))
    side = torch.cuda.Stream(device=dev)
    for call in calls:
        first = call(pos, depth, Kinv, proj)
        assert float(first[1].max()) > 1 and 0 < float(first[0].mean()) < 1
        second = call(pos, depth, Kinv, proj)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            third = call(pos, depth, Kinv, proj)
        side.synchronize()
        flipped = call(*(t.flip(0).contiguous() for t in (pos, depth, Kinv, proj)))
        for other in (second, third, tuple(t.flip(0) for t in flipped)):
            assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


# ---- the loss functions ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stereo():
    """Case a's camera pair with two images that share their coarse structure and a smooth target depth: [2,3,24,40]."""
    c = U.cases()["a"]
    B, (H, W) = 2, U.SHAPES["a"]
    rng = np.random.RandomState(2700)
    coarse = torch.from_numpy(rng.uniform(0, 1, (B, 3, H // 4, W // 4)))
    base = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    src = (0.8 * base + 0.2 * torch.from_numpy(rng.uniform(0, 1, (B, 3, H, W)))).float()
    tgt = (0.8 * base + 0.2 * torch.from_numpy(rng.uniform(0, 1, (B, 3, H, W)))).float()
    depth = torch.from_numpy(c["depth"]) + torch.from_numpy(rng.uniform(0, 0.5, (B, H, W))).float()
    f = 0.75 * W
    intr = torch.tensor([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]]).expand(B, 3, 3).contiguous()
    pose = torch.eye(4)
    pose[0, 3] = -0.54
    visible = torch.from_numpy(1.0 - c["occ64_2"].astype(np.float32))
    return src, tgt, depth, pose.unsqueeze(0), intr, visible


def _warp(img, depth, pose, intr, mode):
    """The HIP inverse warp with the matrices the loss functions form (the closed-form inverse, intr @ pose[:3])."""
    B = img.shape[0]
    return iv.warp_with_matrices(img, depth, lb._inv3(intr).expand(B, 3, 3), torch.matmul(intr, pose[:, :3]).expand(B, 3, 4), mode)


def _rel(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs().clamp(min=1e-30)).max())


def test_rgb_loss_with_a_mask_is_the_composition(dev):
    src, tgt, depth, pose, intr, vis = (t.to(dev) for t in _stereo())
    assert 0 < float((1 - vis).sum())
    warped, valid = _warp(src, depth, pose, intr, "bilinear")
    keep = torch.ones_like(valid)
    keep[:, :int(valid.shape[1] / 3)] = False
    m = (valid & keep).float().unsqueeze(1) * vis
    diff = (tgt * m - warped * m).abs()
    per_item = (diff * m).reshape(2, -1).sum(1) / m.expand_as(diff).reshape(2, -1).sum(1)
    got = lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=vis)
    plain = lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True)
    print("rsc with the mask", got.tolist(), "written out", per_item.tolist(), "without", plain.tolist())
    assert _rel(got, per_item) <= 1e-6 and not torch.equal(got, plain)
    assert torch.equal(lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=vis[:, 0]), got)
    batch = (diff * m).sum() / m.expand_as(diff).sum()
    assert _rel(lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, occlusion=vis), batch) <= 1e-6
    # with the SSIM and the census distance beside it: every piece sees the masked images, the means divide by the masked mean
    mix = lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=vis, ssim_weight=0.4, ternary_weight=0.3)
    pieces = (0.3 * per_item + 0.4 * ops.ssim(warped * m, tgt * m, 1).reshape(2, -1).mean(1) / m.reshape(2, -1).mean(1) +
              0.3 * ops.ternary(warped * m, tgt * m, 1).reshape(2, -1).mean(1) / m.reshape(2, -1).mean(1))
    assert _rel(mix, pieces) <= 1e-6
    # an all-ones mask changes no value; None changes no operation: the bits of the call without the argument
    ones = torch.ones_like(vis)
    assert torch.equal(lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=ones), plain)
    assert torch.equal(lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=None), plain)
    with pytest.raises(RuntimeError, match="no mask input"):
        lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, fused=True, ssim_weight=0.85, occlusion=vis)
    with pytest.raises(RuntimeError, match="occlusion must be"):
        lb.rgb_stereo_consistency_loss(src, tgt, depth, pose, intr, per_item=True, occlusion=vis[:, :, :-1])


def test_depth_loss_with_a_mask_is_the_composition(dev):
    _, _, depth, pose, intr, vis = (t.to(dev) for t in _stereo())
    rng = np.random.RandomState(2701)
    src_depth = (depth + torch.from_numpy(rng.uniform(-0.5, 0.5, tuple(depth.shape))).float().to(dev)).unsqueeze(1)
    src_mask = torch.from_numpy((rng.rand(*depth.shape) < 0.8).astype(np.float32)).to(dev).unsqueeze(1)
    tgt_depth = depth.unsqueeze(1)
    back = torch.linalg.inv_ex(pose).inverse
    moved = (iv.transform_dmap(src_depth[:, 0], back, intr) * src_mask[:, 0]).unsqueeze(1)
    warped, valid = _warp(moved, depth, pose, intr, "nearest")
    keep = torch.ones_like(valid)
    keep[:, :int(valid.shape[1] / 3)] = False
    m = ((valid & keep).unsqueeze(1) & (warped > 0)).float() * vis
    a, b = (tgt_depth * m).clamp(min=1e-3), (warped * m).clamp(min=1e-3)
    diff = ((a - b).abs() / (a + b).abs()).clamp(0, 1)
    per_item = (diff * m).reshape(2, -1).sum(1) / m.reshape(2, -1).sum(1)
    args = (src_depth, tgt_depth, src_mask, None, pose, intr)
    got = lb.depth_stereo_consistency_loss(*args, per_item=True, occlusion=vis)
    plain = lb.depth_stereo_consistency_loss(*args, per_item=True)
    print("dsc with the mask", got.tolist(), "written out", per_item.tolist(), "without", plain.tolist())
    assert _rel(got, per_item) <= 1e-6 and not torch.equal(got, plain)
    assert torch.equal(lb.depth_stereo_consistency_loss(*args, per_item=True, occlusion=vis[:, 0]), got)
    assert torch.equal(lb.depth_stereo_consistency_loss(*args, per_item=True, occlusion=None), plain)
    assert torch.equal(lb.depth_stereo_consistency_loss(*args, pose_src2target=back, per_item=True, occlusion=torch.ones_like(vis)), plain)


# ---- BaseLoss -------------------------------------------------------------------------------------------------------------------------
def _cfg(**loss):
    cfg = util_loss.loss_cfg()
    cfg.loss.__dict__.update(loss)
    return cfg


def _run(dev, cfg, backward=True, **how):
    output, target = util_loss.structure(util_loss.make_inputs(), img_utils.gen_soft_label_torch, dev=dev)
    loss = BaseLoss(cfg, 0, **how)(output, target)
    if backward:
        loss.backward()
    return loss.detach(), [v.grad for v in util_loss.volumes(output)], (output, target)


@pytest.mark.parametrize("fused_terms", (False, True))
@pytest.mark.parametrize("fused_photo", (False, True))
def test_base_loss_without_the_key_keeps_its_bits(dev, monkeypatch, fused_terms, fused_photo):
    """occ absent = occ 0, bit for bit, and the op is not called: the loss with every term on; the gradients with dsc off (its
    source gradient is summed with float atomics, whose last bits differ from run to run with or without the key)."""
    calls = []
    real = _native.depth_range_map
    monkeypatch.setattr(_native, "depth_range_map", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    how = dict(fused_terms=fused_terms, fused_photo=fused_photo)
    for extra in ({}, {"rsc_ssim": 0.85}):
        on = dict(rsc_low_mul=1.0, **extra)
        assert torch.equal(_run(dev, _cfg(**on), backward=False, **how)[0], _run(dev, _cfg(occ=0, occ_th=0.5, **on), backward=False, **how)[0])
        absent = _run(dev, _cfg(dsc_mul=0.0, **on), **how)
        zero = _run(dev, _cfg(dsc_mul=0.0, occ=0, occ_th=0.5, **on), **how)
        assert torch.equal(absent[0], zero[0]) and all(torch.equal(a, b) for a, b in zip(absent[1], zero[1]))
    assert calls == []


def _regressed_depths(output, target):
    """The depth maps BaseLoss regresses from the last volumes (ops.dpv_soft_ce), {side: {hi: map}}."""
    dc = target[0]["d_candi"]
    out = {}
    for s, o, tg in (("l", output[0], target[0]), ("r", output[1], target[1])):
        out[s] = {True: ops.dpv_soft_ce(o["output_refined"][-1], dc, mask=tg["masks_imgsizes"][:, 0], want_depth=True,
                                        label=torch.stack(list(tg["soft_labels_imgsize"])))[1],
                  False: ops.dpv_soft_ce(o["output"][-1], dc, mask=tg["masks"][:, 0], want_depth=True,
                                         label=torch.stack(list(tg["soft_labels"])))[1]}
    return out


def _cameras(target, dev):
    tl, tr = target
    T = tl["T_left2right"].float()
    l2r, r2l = T.unsqueeze(0).to(dev), torch.inverse(T).unsqueeze(0).to(dev)

    def camera(intr, pose):
        k = intr.float()
        B = k.shape[0]
        return lb._inv3(k).expand(B, 3, 3), torch.matmul(k, pose[:, 0:3, :].float()).expand(B, 3, 4)
    return l2r, r2l, camera


def test_base_loss_with_the_masks(dev, monkeypatch):
    """occ = 1 with rsc, rsc_low and dsc on: the loss is the sum of the loss_blocks calls with the four masks, over 2 B, whatever
    fused_terms and fused_photo say (four calls of the op per forward)."""
    three = dict(ce_mul=0.0, dc_mul=0.0, smooth_mul=0.0, dsc_mul=1.0, rsc_mul=1.0, rsc_low_mul=1.0)
    calls = []
    real = _native.depth_range_map
    monkeypatch.setattr(_native, "depth_range_map", lambda *a, **k: (calls.append(k.get("th")), real(*a, **k))[1])
    loss, grads, (output, target) = _run(dev, _cfg(occ=1, occ_th=0.5, **three))
    assert calls == [0.5] * 4
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    plain = _run(dev, _cfg(**three), backward=False)[0]
    assert len(calls) == 4 and not torch.equal(plain, loss)
    tl, tr = target
    l2r, r2l, camera = _cameras(target, dev)
    with torch.no_grad():
        d = _regressed_depths(output, target)
        rgb = {True: (tl["rgb"][:, -1], tr["rgb"][:, -1])}
        rgb[False] = tuple(torch.nn.functional.interpolate(t, scale_factor=0.25, mode="bilinear") for t in rgb[True])
        dsc = rsc = rsc_low = 0
        removed = 0
        for hi in (True, False):
            ik, mk = ("intrinsics_up", "masks_imgsizes") if hi else ("intrinsics", "masks")
            vis_l = ops.depth_occlusion(d["r"][hi], *camera(tr[ik], r2l), th=0.5)
            vis_r = ops.depth_occlusion(d["l"][hi], *camera(tl[ik], l2r), th=0.5)
            removed += int((vis_l == 0).sum()) + int((vis_r == 0).sum())
            dl, dr = d["l"][hi].unsqueeze(1), d["r"][hi].unsqueeze(1)
            dsc = dsc + lb.depth_stereo_consistency_loss(dr, dl, tr[mk], tl[mk], l2r, tl[ik], pose_src2target=r2l, per_item=True,
                                                         occlusion=vis_l).sum()
            dsc = dsc + lb.depth_stereo_consistency_loss(dl, dr, tl[mk], tr[mk], r2l, tr[ik], pose_src2target=l2r, per_item=True,
                                                         occlusion=vis_r).sum()
            il, ir = rgb[hi]
            term = (lb.rgb_stereo_consistency_loss(ir, il, d["l"][hi], l2r, tl[ik], per_item=True, occlusion=vis_l).sum() +
                    lb.rgb_stereo_consistency_loss(il, ir, d["r"][hi], r2l, tr[ik], per_item=True, occlusion=vis_r).sum())
            if hi:
                rsc = term
            else:
                rsc_low = term
        bsize = float(2 * util_loss.B)
        want = dsc / bsize + rsc / bsize + rsc_low / bsize
    print("BaseLoss with the masks", float(loss), "the functions", float(want), "without the masks", float(plain), "pixels removed", removed)
    assert removed > 0
    assert _rel(loss, want) <= 1e-6
    for how in ({"fused_terms": True}, {"fused_photo": True}, {"fused_terms": True, "fused_photo": True}):
        del calls[:]
        again = _run(dev, _cfg(occ=1, occ_th=0.5, rsc_ssim=0.0, **three), backward=False, **how)[0]
        assert calls == [0.5] * 4 and torch.equal(again, loss), how
    # the threshold defaults to 0.2; the other fused terms stay fused
    del calls[:]
    every = _run(dev, _cfg(occ=1, rsc_low_mul=1.0, rsc_ssim=0.85), fused_terms=True, fused_photo=True)
    assert calls == [0.2] * 4 and bool(torch.isfinite(every[0]))
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in every[1])


def test_base_loss_masked_pixels_get_no_rsc_gradient(dev):
    """Only rsc_mul on: a pixel of the target depth map reaches the loss through its own sample alone, so where the mask is 0 the
    gradient of every plane of the refined volume is exactly 0 -- and without the masks some of those pixels have one."""
    only = dict(ce_mul=0.0, dsc_mul=0.0, dc_mul=0.0, smooth_mul=0.0, rsc_low_mul=0.0, rsc_mul=1.0)
    loss, grads, (output, target) = _run(dev, _cfg(occ=1, occ_th=0.5, **only))
    _, g_plain, _ = _run(dev, _cfg(**only))
    tl, tr = target
    l2r, r2l, camera = _cameras(target, dev)
    with torch.no_grad():
        d = _regressed_depths(output, target)
        gone = {1: ops.depth_occlusion(d["r"][True], *camera(tr["intrinsics_up"], r2l), th=0.5) == 0,    # left refined volume
                3: ops.depth_occlusion(d["l"][True], *camera(tl["intrinsics_up"], l2r), th=0.5) == 0}    # right refined volume
    assert bool(torch.isfinite(loss))
    for at, mask in gone.items():
        mask = mask.expand_as(grads[at])
        assert int(mask.sum()) > 0
        assert int(torch.count_nonzero(grads[at][mask])) == 0
        assert int(torch.count_nonzero(g_plain[at][mask])) > 0
        assert int(torch.count_nonzero(grads[at][~mask])) > 0
    assert grads[0] is None or int(torch.count_nonzero(grads[0])) == 0   # the low-resolution volumes are not in this loss
