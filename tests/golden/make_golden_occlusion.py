"""Golden fixture g27_occlusion: the reference's range map and occlusion masks (utils/warp_utils.py) and the positions of its own
pixel2cam / cam2pixel (utils/inverse_warp.py) on the CPU.  Build container only (imports the reference, which never travels):

    python tests/golden/make_golden_occlusion.py

Inputs: tests/util_occlusion.py -- the depth cases a-d (scene) and the generic flows e_* on 16 x 16 (flows), B = 2 throughout.
Stored per depth case: depth, Kinv, proj (c: also holes, and the depth map before the holes), the reference's positions in float32
and float64 (pos32; pos64 as pos64_minus_pos32 in float32, util_occlusion.pos64 puts it back), its get_corresponding_map on them (r32, r64), its get_occu_mask_backward at th 0.2 and 0.5 (occ32_*,
occ64_*, uint8), and e32 = max |r32 - r64|.  Per flow case: the flow and the same outputs (e_nonfinite: the flow alone -- the
reference's .long() of a NaN is undefined).  flowpair: x, flow12, flow21 and the reference's flow_warp (border, zeros) and
get_occu_mask_bidirection.

Checked here: the float64 restatement of tests/util_occlusion.py agrees with the reference run in float64 to 1e-12, positions and
range maps; and NO pixel of any case has clamp(r, 0, 1) within util_occlusion.MARGIN of a threshold in float64 -- neither the range
map of the float64 positions nor that of the float32 positions -- a condition on the inputs, not a tolerance: a seed that breaks it
is changed (util_occlusion.SEEDS).  The flow cases have dyadic weights: a sum of sixteenths can be exactly 0.5, so there the
condition is that the range map is the same number in float32 and float64 (asserted, reference and restatement) and that every
pixel that is not exactly 0.5 keeps the margin.  Data only; nothing of the reference is copied.
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util_occlusion as U  # noqa: E402


def _key(th):
    return str(th).replace("0.", "")


def _range_and_masks(wu, pos, out, name, tag):
    """The reference's range map of positions `pos` and its masks through get_occu_mask_backward (flow = pos - base grid)."""
    B, _, H, W = pos.shape
    r = wu.get_corresponding_map(pos)
    out[f"{name}.r{tag}"] = r.numpy()
    flow = pos - U.base_grid(B, H, W, pos.dtype)
    for th in U.THS:
        occ = wu.get_occu_mask_backward(flow, th=th)
        assert torch.equal(occ, (r.clamp(0.0, 1.0) < th).float()), (name, tag, th)   # (base + (pos - base) moves no bit that matters)
        out[f"{name}.occ{tag}_{_key(th)}"] = occ.numpy().astype(np.uint8)
    return r


def _check(name, r64_ref, pos64, pos32, exact=False):
    mine = U.range_map(pos64)
    assert float((mine - r64_ref).abs().max()) <= 1e-12, name
    if exact:   # dyadic weights: a pixel may sit ON a threshold, where float32 and float64 hold the same number and decide alike
        assert torch.equal(mine, U.range_map(pos32).double()), name
        off = mine[(mine != 0.5)]
        m = U.margin(off)
    else:
        m = min(U.margin(mine), U.margin(U.range_map(pos32.double())))
    assert m > U.MARGIN, f"{name}: a pixel lies {m:.2e} from a threshold: change the seed"
    return m


def main():
    _import_reference()
    import utils.inverse_warp as iw
    import utils.warp_utils as wu
    out = {}
    for name in U.DEPTH_CASES:
        depth, Kinv, proj, holes, full = U.scene(name)
        out[f"{name}.depth"], out[f"{name}.Kinv"], out[f"{name}.proj"] = depth, Kinv, proj
        if holes is not None:
            out[f"{name}.holes"], out[f"{name}.depth_full"] = holes.astype(np.uint8), full
        pos = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            d, ki, pr = (torch.from_numpy(v).to(dtype) for v in (depth, Kinv, proj))
            iw.pixel_coords = None   # (the reference caches its pixel grid in the dtype of the first call)
            B, H, W = d.shape
            grid = iw.cam2pixel(iw.pixel2cam(d, ki), pr[:, :, :3], pr[:, :, 3:], "zeros")   # [B,H,W,2], normalised
            xn, yn = grid[..., 0], grid[..., 1]
            pos[tag] = torch.stack((((xn + 1) * W - 1) / 2, ((yn + 1) * H - 1) / 2), 1)     # align_corners=False
        # float64 positions as their float32 distance from the float32 ones (half the bytes; exact to 1e-13 of the largest position)
        out[f"{name}.pos32"] = pos["32"].numpy()
        out[f"{name}.pos64_minus_pos32"] = (pos["64"] - pos["32"].double()).float().numpy()
        back = pos["32"].double() + torch.from_numpy(out[f"{name}.pos64_minus_pos32"]).double()
        assert float((back - pos["64"]).abs().max()) <= 1e-13 * max(1.0, float(pos["64"].abs().max())), name
        mine = U.depth_positions(*(torch.from_numpy(v).double() for v in (depth, Kinv, proj)))
        assert float((mine - pos["64"]).abs().max()) <= 1e-12 * max(1.0, float(pos["64"].abs().max())), name
        r32 = _range_and_masks(wu, pos["32"], out, name, "32")
        r64 = _range_and_masks(wu, pos["64"], out, name, "64")
        m = _check(name, r64, pos["64"], pos["32"])
        e32 = float((r32.double() - r64).abs().max())
        out[f"{name}.e32"] = np.float64(e32)
        occluded = float(out[f"{name}.occ64_2"].mean())
        print(f"{name}: e32 = {e32:.2e}, margin {m:.2e}, occluded at 0.2: {100 * occluded:.1f} %")
    for name in U.FLOW_CASES:
        flow = U.flows(name)
        out[f"{name}.flow"] = flow
        if name == "e_nonfinite":
            continue
        B, _, H, W = flow.shape
        pos32 = U.base_grid(B, H, W) + torch.from_numpy(flow)
        r32 = _range_and_masks(wu, pos32, out, name, "32")
        r64 = _range_and_masks(wu, pos32.double(), out, name, "64")
        m = _check(name, r64, pos32.double(), pos32, exact=True)
        assert torch.equal(r32.double(), r64), name
        print(f"{name}: |r32 - r64| = {float((r32.double() - r64).abs().max()):.2e}, margin {m:.2e}, max r = {float(r64.max()):.0f}")
    x, f12, f21 = U.flow_pair()
    out["flowpair.x"], out["flowpair.flow12"], out["flowpair.flow21"] = x, f12, f21
    tx, t12, t21 = (torch.from_numpy(v) for v in (x, f12, f21))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out["flowpair.warp_border"] = wu.flow_warp(tx, t12).numpy()
        out["flowpair.warp_zeros"] = wu.flow_warp(tx, t12, pad="zeros").numpy()
        out["flowpair.bidirection"] = wu.get_occu_mask_bidirection(t12, t21).numpy().astype(np.uint8)
    print("bidirection: occluded %.1f %%" % (100 * float(out["flowpair.bidirection"].mean())))
    path = os.path.join(HERE, "g27_occlusion.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
