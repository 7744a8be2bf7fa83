"""Backward time of warp_feature at the feedback model's call (B = 4, V + 1 = 2, D = 64, 64 x 128), both paths of
csrc/warp_bwd.hip, against the only "before" there is: a torch composite on the same GPU (per (item, view) F.grid_sample on
src[b, v] viewed as [D,1,H,W] with the oracle's plane_coords grid, under PyTorch-ROCm autograd).

    python tools/bench_warp_backward.py [--reps 50] [--warmup 5] [--burst 20]

Prints ONE JSON line.  Per variant, device events after --warmup calls:
  *_ms        median over --reps of the events around ONE call (the Python wrapper's launches and allocations included);
  *_burst_ms  median over --reps // 5 windows of --burst calls enqueued back to back, per call: what the device needs per call
              when the queue is kept full (or the host's enqueue rate, where that is the slower one);
variants: fwd (ops.warp_feature under no_grad), atomic / det (_native.warp_feature_backward: clear + scatter; clear + maximum +
integer scatter + convert, the workspace allocation included), torch_fwd / torch_bwd (the composite: forward under autograd,
out.backward(g) on a retained graph).  Also: atomic_bytes, the bytes the atomic path adds (4 bytes per in-bounds tap, counted on
the sample positions of the call), max_rel_diff between the two paths and between the atomic path and the composite, and
workspace_bytes.  No threshold: the numbers are a record."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import _native, ops, synth  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

SHAPE = dict(B=4, V=2, D=64, H=64, W=128, pose="mono")


def timed(fn, reps, warmup, burst=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / burst)
    return float(np.median(ms))


def composite(src, d, dc):
    B, V, D, H, W = src.shape
    out = []
    for i in range(B):
        for v in range(V):
            grid = O.plane_coords(d["K"][i], d["R"][i, v], d["t"][i, v], d["rays"][i], dc, d["cxcy"][i, 0], d["cxcy"][i, 1]).reshape(D, H, W, 2)
            out.append(F.grid_sample(src[i, v].unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0])
    return torch.stack(out).reshape(B, V, D, H, W)


def in_bounds_taps(d, dc, s):
    ix, iy = ops.sample_coords(d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc, s["H"], s["W"])
    x0, y0 = torch.floor(ix), torch.floor(iy)
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    nx = ((x0 >= 0) & (x0 < s["W"])).int() + ((x0 + 1 >= 0) & (x0 + 1 < s["W"])).int()
    ny = ((y0 >= 0) & (y0 < s["H"])).int() + ((y0 + 1 >= 0) & (y0 + 1 < s["H"])).int()
    return int((nx * ny * fin.int()).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = SHAPE
    b = synth.make_batch(77, s["B"], C=s["D"], D=s["D"], H=s["H"], W=s["W"], V=s["V"], pose=s["pose"])
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    dc = ops.d_candi_tensor(d["d_candi"], dev)
    cam = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc)
    src = d["src"]
    g = torch.randn(src.shape, device=dev)
    run = {
        "fwd": lambda: ops.warp_feature(src, *cam),
        "atomic": lambda: _native.warp_feature_backward(g, *cam, deterministic=False),
        "det": lambda: _native.warp_feature_backward(g, *cam, deterministic=True),
    }
    leaf = src.clone().requires_grad_(True)
    tout = composite(leaf, d, dc)
    run["torch_fwd"] = lambda: composite(leaf, d, dc)
    run["torch_bwd"] = lambda: torch.autograd.backward(tout, g, retain_graph=True)
    out = {"device": torch.cuda.get_device_name(0), "shape": s}
    with torch.no_grad():
        for name in ("fwd", "atomic", "det"):
            out[name + "_ms"] = round(timed(run[name], a.reps, a.warmup), 4)
            out[name + "_burst_ms"] = round(timed(run[name], max(3, a.reps // 5), 1, a.burst), 4)
    for name in ("torch_fwd", "torch_bwd"):
        out[name + "_ms"] = round(timed(run[name], a.reps, a.warmup), 4)
        out[name + "_burst_ms"] = round(timed(run[name], max(3, a.reps // 5), 1, a.burst), 4)
        leaf.grad = None
    ga, gd = run["atomic"](), run["det"]()
    run["torch_bwd"]()
    desc = _native.SweepDesc(s["B"], s["V"], s["D"], s["D"], s["H"], s["W"], 0, 0, 0, 1.0, 0, 0, 0)
    out.update(atomic_bytes=4 * in_bounds_taps(d, dc, s), samples=src.numel(),
               workspace_bytes=int(_native.load().pdepth_warp_feature_backward_det_workspace_bytes(ctypes.byref(desc))),
               max_rel_diff_det_atomic=float((ga - gd).abs().max() / ga.abs().max()),
               max_rel_diff_atomic_torch=float((ga - leaf.grad).abs().max() / ga.abs().max()),
               same_bits_twice=bool(torch.equal(gd, run["det"]())))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
