"""Shared by the suites of the sweep backward (csrc/sweep_bwd.hip): autograd of the oracle's formula in float64 / fp32, the
HIP gradients, the error measure and its L1 allowance; and a host restatement of how the g_src pass of the kernel groups the
planes of a (tile, view) pair -- staged through the LDS box image, added directly, or empty -- with the inputs that reach the
paths the ordinary poses never take (tests/test_sweep_backward_groups.py)."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from pdepth_amd import ops, synth
from oracle import ref_cpu as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(REPO, "probabilistic-depth_amd", "csrc", "sweep_bwd_body.hpp")   # the one body of both g_src paths


def to_dev(b, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def oracle_cost(ref, src, b, sigma, metric, dtype):
    """est_swp_volume_v4 restated on device tensors of `dtype` (grid from oracle.ref_cpu.plane_coords, fp32, cast) -> [B,D,H,W]."""
    B, V, C, H, W = src.shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    D = d32.numel()
    out = []
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        cost = 0
        for v in range(V):
            grid = O.plane_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), d32, cx, cy).reshape(D, H, W, 2)
            grid = grid.to(device=src.device, dtype=dtype)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                                   align_corners=False)
            diff = warped - ref[i].unsqueeze(0)
            dist = (diff ** 2).sum(1) if metric == "L2" else diff.abs().sum(1)
            cost = cost + dist / sigma
        out.append(cost)
    return torch.stack(out)


def oracle_grads(b, gup, sigma, metric, dtype, dev):
    ref = b["ref"].to(dev, dtype).detach().clone().requires_grad_(True)
    src = b["src"].to(dev, dtype).detach().clone().requires_grad_(True)
    (oracle_cost(ref, src, b, sigma, metric, dtype) * gup.to(dtype)).sum().backward()
    return ref.grad, src.grad


def hip_grads(d, gup, sigma, metric, algo="auto", want_ref=True, want_src=True):
    """(g_ref, g_src, cost) of ops.sweep_cost; an output that is not wanted (its input does not require grad) is None."""
    ref = d["ref"].clone().requires_grad_(want_ref)
    src = d["src"].clone().requires_grad_(want_src)
    cost = ops.sweep_cost(ref, src, d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], sigma, feat_dist=metric, algo=algo)
    (cost * gup).sum().backward()
    return ref.grad, src.grad, cost


def rel_err(g, g64, allow=None, den=None):
    """max |g - g64| / max |g64|; with `allow`, the excess over the per-element allowance (see l1_allowance); with `den`, that
    denominator instead (a part of a tensor measured against the maximum of the whole)."""
    d = (g.double() - g64).abs()
    if allow is not None:
        d = (d - allow).clamp_min(0)
    return float(d.max() / (g64.abs().max() if den is None else den))


def l1_allowance(b, gup, sigma, dev, tau=1e-5):
    """(allow_ref, allow_src): how far a correct fp32 evaluation of the L1 gradient may be from the float64 one.

    d|e|/de = sign(e) jumps at e = 0.  Where the float64 difference e of a (view, plane, pixel, channel) sample is within
    fp32 rounding of zero (|e| <= tau (1 + |ref|): some ten times the fp32 error of e), an fp32 evaluation may take the other
    branch -- sign +-1 or 0 instead of the float64 one --, a change of up to 2 g / sigma in g_ref and 2 g w_t / sigma in g_src
    at the sample's taps (about one sample in 1e5 at the shapes below).  The allowance is exactly that bound, summed over the
    ambiguous samples; every other element is held to the plain criterion."""
    dt = torch.float64
    ref = b["ref"].to(dev, dt)
    src = b["src"].to(dev, dt).detach().clone().requires_grad_(True)
    B, V, C, H, W = src.shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    D = d32.numel()
    g = gup.to(dev, dt).abs() * (2.0 / sigma)
    allow_ref = torch.zeros_like(ref)
    total = 0
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            grid = O.plane_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), d32, cx, cy).reshape(D, H, W, 2)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid.to(dev, dt), mode="bilinear",
                                   padding_mode="zeros", align_corners=False)
            amb = ((warped.detach() - ref[i].unsqueeze(0)).abs() <= tau * (1 + ref[i].abs().unsqueeze(0))).to(dt)
            w = amb * g[i].unsqueeze(1)                                     # [D,C,H,W]
            allow_ref[i] += w.sum(0)
            total = total + (w * warped).sum()                              # d/dsrc = the taps' weights times w
    total.backward()
    return allow_ref, src.grad


# ---- the plane groups of the g_src pass, restated on the host ------------------------------------------------------------
def kernel_constants():
    """(BOX_CAP, BT) as csrc/sweep_bwd_body.hpp declares them: the cases below are chosen against these two numbers."""
    text = open(KERNEL).read()
    found = []
    for name in ("BOX_CAP", "BT"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, "csrc/sweep_bwd_body.hpp no longer declares 'constexpr int %s = <number>;'" % name
        found.append(int(m.group(1)))
    return tuple(found)


_BIG = 1 << 30


def plane_boxes(ix, iy, H, W, tile):
    """Per plane and tile, the box of the in-bounds taps of the tile's live pixels: (x_lo, x_hi, y_lo, y_hi), each an int64
    array [D, tiles_y, tiles_x]; no in-bounds tap: x_lo > x_hi.  A tap is one of the four texels (floor(ix) + {0, 1},
    floor(iy) + {0, 1}); it is in bounds when it lies in [0, W) x [0, H) and the position is finite."""
    ix, iy = np.asarray(ix, dtype=np.float32).reshape(-1, H, W), np.asarray(iy, dtype=np.float32).reshape(-1, H, W)
    finite = np.isfinite(ix) & np.isfinite(iy)
    with np.errstate(invalid="ignore"):
        x0 = np.clip(np.floor(np.where(finite, ix, -2.0)), -2, W + 1).astype(np.int64)   # (beyond -2 / size + 1: out anyway)
        y0 = np.clip(np.floor(np.where(finite, iy, -2.0)), -2, H + 1).astype(np.int64)
    xin0, xin1 = finite & (x0 >= 0) & (x0 < W), finite & (x0 + 1 >= 0) & (x0 + 1 < W)
    yin0, yin1 = finite & (y0 >= 0) & (y0 < H), finite & (y0 + 1 >= 0) & (y0 + 1 < H)
    any_x, any_y = xin0 | xin1, yin0 | yin1
    lo_hi = (np.where(xin0 & any_y, x0, np.where(xin1 & any_y, x0 + 1, _BIG)),
             np.where(xin1 & any_y, x0 + 1, np.where(xin0 & any_y, x0, -_BIG)),
             np.where(yin0 & any_x, y0, np.where(yin1 & any_x, y0 + 1, _BIG)),
             np.where(yin1 & any_x, y0 + 1, np.where(yin0 & any_x, y0, -_BIG)))
    ty, tx = -(-H // tile), -(-W // tile)
    out = []
    for j, a in enumerate(lo_hi):
        fill = _BIG if j % 2 == 0 else -_BIG
        pad = np.full((a.shape[0], ty * tile, tx * tile), fill, dtype=np.int64)
        pad[:, :H, :W] = a
        pad = pad.reshape(-1, ty, tile, tx, tile)
        out.append(pad.min(axis=(2, 4)) if j % 2 == 0 else pad.max(axis=(2, 4)))
    return tuple(out)


def _union(u, box):
    return (min(u[0], box[0]), max(u[1], box[1]), min(u[2], box[2]), max(u[3], box[3]))


def box_area(box):
    return (box[1] - box[0] + 1) * (box[3] - box[2] + 1) if box[0] <= box[1] else 0


def group_planes(boxes, cap):
    """The groups of one (tile, view) pair from its per-plane boxes, greedy as the kernel forms them: extend the group while
    the union of the boxes has at most `cap` texels (a plane with no in-bounds tap adds nothing to the union).
    -> list of ("staged", k0, k1, box), ("direct", k, box) -- a plane whose own box exceeds the cap --, ("empty", k0, k1):
    planes k0 <= k < k1, box = (x_lo, x_hi, y_lo, y_hi) inclusive."""
    none = (_BIG, -_BIG, _BIG, -_BIG)
    out, k, D = [], 0, len(boxes)
    while k < D:
        u, k1 = none, k
        while k1 < D:
            n = _union(u, boxes[k1])
            if box_area(n) > cap:
                break
            u, k1 = n, k1 + 1
        if k1 == k:
            out.append(("direct", k, tuple(int(x) for x in boxes[k])))
            k1 = k + 1
        elif u[0] <= u[1]:
            out.append(("staged", k, k1, tuple(int(x) for x in u)))
        else:
            out.append(("empty", k, k1))
        k = k1
    return out


def tile_groups(b, cap, tile):
    """{(item, view, tile_y, tile_x): groups (see group_planes)} for a batch dict of synth.make_batch: what the g_src pass of
    csrc/sweep_bwd.hip does with every (tile, view) pair, from the sample positions of oracle.ref_cpu.sample_coords."""
    B, V, C, H, W = b["src"].shape
    out = {}
    for i in range(B):
        K = b["K"][i]
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            ix, iy = O.sample_coords(K, b["R"][i, v], b["t"][i, v], b["rays"][i], b["d_candi"], cx, cy, H, W)
            x_lo, x_hi, y_lo, y_hi = plane_boxes(ix.numpy(), iy.numpy(), H, W, tile)
            for ty in range(x_lo.shape[1]):
                for tx in range(x_lo.shape[2]):
                    boxes = [(x_lo[k, ty, tx], x_hi[k, ty, tx], y_lo[k, ty, tx], y_hi[k, ty, tx]) for k in range(x_lo.shape[0])]
                    out[(i, v, ty, tx)] = group_planes(boxes, cap)
    return out


def pair_box(groups):
    """The union of the boxes of a pair's staged groups and direct planes, or None."""
    u = (_BIG, -_BIG, _BIG, -_BIG)
    for g in groups:
        if g[0] != "empty":
            u = _union(u, g[-1])
    return u if u[0] <= u[1] else None


def describe(groups):
    def one(g):
        if g[0] == "staged":
            return "staged[%d:%d] x %d..%d y %d..%d (%d texels)" % (g[1], g[2], *g[3], box_area(g[3]))
        if g[0] == "direct":
            return "direct[%d] x %d..%d y %d..%d (%d texels)" % (g[1], *g[2], box_area(g[2]))
        return "empty[%d:%d]" % (g[1], g[2])
    return ", ".join(one(g) for g in groups)


def group_stats(tg, C, channels_per_pass=8):
    """The counts that the coverage test holds the cases to."""
    kinds = {key: [g[0] for g in gs] for key, gs in tg.items()}
    follows = sum(1 for ks in kinds.values() for a, b_ in zip(ks, ks[1:]) if a == "empty" and b_ in ("direct", "staged"))
    return {"pairs": len(tg),
            "staged": sum(ks.count("staged") for ks in kinds.values()),
            "direct": sum(ks.count("direct") for ks in kinds.values()),
            "direct_with_channel_tail": sum(ks.count("direct") for ks in kinds.values()) if C % channels_per_pass else 0,
            "pairs_3_groups": sum(1 for ks in kinds.values() if len(ks) >= 3),
            "pairs_split_no_direct": sum(1 for ks in kinds.values() if ks.count("staged") >= 2 and "direct" not in ks),
            "pairs_all_empty": sum(1 for ks in kinds.values() if set(ks) == {"empty"}),
            "empty_then_group": follows}


def _zoom_case(config_id, C, H, W, V, d_lo, d_hi, ts, B=1, roll_deg=None):
    """make_batch(..., D = 16, pose 'mono') with R, t and d_candi overwritten: R = a roll about the optical axis (identity
    without one), t as given per (item, view).  min(d_candi) + t_z >= 1: no plane comes near the camera plane."""
    b = synth.make_batch(config_id, B, C=C, D=16, H=H, W=W, V=V, pose="mono")
    b["d_candi"] = synth.powerf(d_lo, d_hi, 16, 1.0)
    t = torch.tensor(ts, dtype=torch.float32).reshape(B, V, 3)
    assert float(b["d_candi"].min() + t[..., 2].min()) >= 1.0
    R = torch.eye(3).repeat(B, V, 1, 1)
    if roll_deg is not None:
        for i in range(B):
            for v in range(V):
                a = np.deg2rad(roll_deg[i][v])
                R[i, v] = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    b["R"], b["t"] = R, t
    return b


def group_cases():
    """name -> batch dict.  The source camera stands in FRONT of the reference one (t_z < 0), so the warp magnifies: the taps
    of a 16 x 16 tile of near planes spread over more texels than the LDS box image holds.

    A: 72 x 88 (ragged in both directions: 8 live rows and columns in the last tiles), C = 11 (3 live channels in the second
       channel pass).  View 0 zooms 5x on the nearest plane, 1.5x on the farthest; the tile that holds the principal point
       spreads into all four quadrants and goes over the cap.  View 1 is a lateral baseline that pushes whole tiles out of
       the image.
    C: 88 x 104, one view, a milder zoom: a pair splits into two staged groups, no direct plane.
    E: 72 x 120, one view, planes 5 ... 20 m apart by 1 m: the lateral baseline throws the nearest plane of the leftmost middle
       tile out of the image altogether and the next one back into it at 3x, whole: an empty run, then a direct plane.
    R: two items of two views, 80 x 120, each view rolled about the optical axis by another angle: the boxes of a rolled
       tile are wider than the tile's footprint, more pairs split, and the second item's outputs lie behind the first's."""
    return {
        "A": _zoom_case(41, 11, 72, 88, 2, 5.0, 12.0, [[(0.3, 0.1, -4.0), (9.0, 0.0, 0.5)]]),
        "C": _zoom_case(42, 5, 88, 104, 1, 4.0, 10.0, [[(0.5, 0.2, -2.6)]]),
        "E": _zoom_case(44, 11, 72, 120, 1, 5.0, 20.0, [[(5.2, -0.2, -4.0)]]),
        "R": _zoom_case(43, 9, 80, 120, 2, 5.0, 12.0, [[(0.3, 0.1, -3.5), (-0.4, 0.2, -2.0)], [(6.0, -0.3, -3.0), (0.0, 0.0, -4.0)]],
                        B=2, roll_deg=[[35.0, -20.0], [10.0, 45.0]]),
    }
