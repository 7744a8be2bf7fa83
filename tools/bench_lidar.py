"""Time of the LiDAR ground-truth call (ops.lidar_depth: csrc/lidar_depth.hip) against what a user could write without it: a
torch composition on the device -- matmul for the transform and the projection, scatter_reduce(amin) for the z-buffer, pooling ops
for the occlusion filter and the 4x4 min-pool.

    python tools/bench_lidar.py [--shapes train,single] [--reps 200] [--warmup 10] [--rounds 3]

Prints ONE JSON line: per shape the median over --reps calls (device events around each call, after --warmup calls; the two sides
alternate --rounds times and the samples of all rounds are pooled) of
  fused_us    : ops.lidar_depth (three launches);
  composed_us : the torch composition below (no host synchronisation either);
  ratio       : composed_us / fused_us;
  differing_pixels : full-resolution pixels whose non-zero pattern differs between the two (the composition's matmul sums in another
                order, so a point on a pixel boundary may land next door), of `shown_pixels` non-zero ones.
Both are timed as a user calls them, allocation of the outputs included.  It gates nothing.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import ops  # noqa: E402

# name -> (B, points per item, H, W, filtering): the training shape of the KITTI configurations, and one item of it
SHAPES = {"train": (8, 125000, 256, 768, 2), "single": (1, 125000, 256, 768, 2)}


def scan(B, n, H, W, dev, seed=5):
    """B scans of a 64-beam sensor (a full turn; ground plane and walls of a random range per azimuth sector) with a KITTI-like
    calibration -> points [B,n,4], counts [B] (a few rows short of n), M [4,4], intr [3,4]."""
    g = torch.Generator().manual_seed(seed)
    beam = torch.randint(0, 64, (B, n), generator=g).double()
    elev = torch.deg2rad(2.0 - 26.8 * beam / 63.0)
    az = (torch.rand(B, n, generator=g).double() * 2 - 1) * math.pi
    sectors = 4.0 + 56.0 * torch.rand(B, 96, generator=g).double()
    wall = torch.gather(sectors, 1, ((az + math.pi) / (2 * math.pi) * 96).long().clamp(0, 95))
    ground = torch.where(elev < 0, 1.73 / (-torch.sin(elev)).clamp_min(1e-9), torch.full_like(elev, float("inf")))
    r = torch.minimum(wall / torch.cos(elev), ground) * (1.0 + 0.002 * torch.randn(B, n, generator=g).double())
    pts = torch.stack([r * torch.cos(elev) * torch.cos(az), r * torch.cos(elev) * torch.sin(az), r * torch.sin(elev), torch.ones_like(r)], 2)
    M = torch.tensor([[0.0, -1.0, 0.0, -0.004], [0.0, 0.0, -1.0, -0.0763], [1.0, 0.0, 0.0, -0.2718], [0.0, 0.0, 0.0, 1.0]])
    fx = 0.58 * W
    intr = torch.tensor([[fx, 0.0, 0.5 * W + 0.7, 0.0585 * fx], [0.0, fx, 0.5 * H + 0.3, 0.0], [0.0, 0.0, 1.0, 0.0027]])
    counts = torch.tensor([n - 17 * b for b in range(B)], dtype=torch.int32)
    return pts.float().to(dev), counts.to(dev), M.to(dev), intr.to(dev)


def composed(points, counts, M, intr, W, H, f, filterdiff=1.0, default=1000.0):
    """The same four tensors from torch ops alone."""
    B, N, _ = points.shape
    cam = points @ M.T
    proj = cam @ intr.T
    z = cam[..., 2]
    u = (proj[..., 0] / proj[..., 2]).double() - 0.5
    v = (proj[..., 1] / proj[..., 2]).double() - 0.5
    ok = (torch.arange(N, device=points.device)[None] < counts[:, None]) & (z >= 0.1) & torch.isfinite(z)
    ok = ok & (u > -1) & (u < W) & (v > -1) & (v < H)
    pix = torch.where(ok, v.trunc().long() * W + u.trunc().long(), H * W)   # (the rejected points go to a slot behind the image)
    inf = torch.full((B, H * W + 1), float("inf"), device=points.device)
    zb = inf.scatter_reduce(1, pix, torch.where(ok, z, float("inf")), "amin")[:, :H * W].view(B, 1, H, W)
    nearest = -F.max_pool2d(-zb, 2 * f + 1, stride=1, padding=f)
    keep = torch.isfinite(zb) & ~((nearest - zb) < -filterdiff)
    keep[:, :, :f] = False
    keep[:, :, H - f - 1:] = False
    keep[:, :, :, :f] = False
    keep[:, :, :, W - f - 1:] = False
    large = torch.where(keep, zb, 0.0)
    mask = (large >= 0.01).float()
    large = large * mask
    small = -F.max_pool2d(-torch.where(large == 0, default, large), 4)
    small = torch.where(small == default, 0.0, small)
    mask_s = (small >= 0.01).float()
    return {"dmap_imgsizes": large[:, 0], "masks_imgsizes": mask, "dmaps": (small * mask_s)[:, 0], "masks": mask_s}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def bench_shape(shape, reps, warmup, rounds, dev):
    B, n, H, W, f = shape
    pts, counts, M, intr = scan(B, n, H, W, dev)
    sides = {"fused_us": lambda: ops.lidar_depth(pts, counts, M, intr, W, H, filtering=f),
             "composed_us": lambda: composed(pts, counts, M, intr, W, H, f)}
    a, b = sides["fused_us"](), sides["composed_us"]()
    out = {"shape": list(shape), "shown_pixels": int((a["dmap_imgsizes"] != 0).sum()),
           "differing_pixels": int(((a["dmap_imgsizes"] != 0) != (b["dmap_imgsizes"] != 0)).sum())}
    pooled = {k: [] for k in sides}
    with torch.no_grad():
        for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on both alike
            for k, fn in sides.items():
                pooled[k] += timed(fn, reps, warmup)
    for k, v in pooled.items():
        out[k] = round(float(np.median(v)), 1)
        out[k.replace("_us", "_p10_p90_us")] = [round(float(np.percentile(v, q)), 1) for q in (10, 90)]
    out["ratio"] = round(out["composed_us"] / out["fused_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="train,single")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lidar: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        out[name] = bench_shape(SHAPES[name], a.reps, a.warmup, a.rounds, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
