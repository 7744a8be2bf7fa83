"""Forward and backward time of the plane sweep under autograd (ops.sweep_cost: csrc/sweep_bwd.hip), against the same math
as PyTorch-ROCm autograd on the GPU (the oracle's formula: plane_coords grid + F.grid_sample + distance, on device tensors).

    python tools/bench_backward.py [--shapes headline,training,config5] [--reps 20] [--warmup 3]
    python tools/bench_backward.py --deterministic [--reps 50]

Prints ONE JSON line: per shape the median over --reps calls (device events, after --warmup calls) of
  fwd_ms / bwd_ms      : ops.sweep_cost with features that require grad / cost.backward(g_cost) (g_ref and g_src);
  torch_fwd_ms / torch_bwd_ms : the comparator; it runs view by view and in chunks of planes (config 5's full repeat of the
                         source would be 18 GB per view): the gradients are the sums over the chunks, the time the sum of theirs;
  atomic_bytes         : bytes the g_src pass adds to global memory with float atomics (upper bound: the box images of the
                         plane groups of every 16 x 16 tile, C channels; texels the group never touched are skipped at run time,
                         planes whose box does not fit add their taps directly), from the shapes and the grouping rule of the
                         kernel evaluated on the sample positions of the call.

--deterministic: ONE JSON line with, per shape (B = 4, V = 1, C = 67, D = 64 at 64 x 128 -- the sweep a model step runs -- and at
256 x 512), the g_src pass alone (_native.sweep_backward, want_ref=False) of the float-atomic path (csrc/sweep_bwd.hip) and of the
deterministic one (csrc/sweep_bwd_det.hip: clear + bounds pre-pass + scatter + convert, the workspace allocation included) in the
same run, the two alternating call by call: atomic_ms / det_ms = medians over --reps calls each (device events), workspace_bytes,
and max_rel_diff between the two results.
"""
import argparse
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

SHAPES = {
    "headline": dict(B=4, V=1, C=67, D=64, H=256, W=512, pose="mono"),
    "training": dict(B=2, V=1, C=67, D=64, H=64, W=96, pose="mono"),
    "config5": dict(B=1, V=4, C=67, D=128, H=512, W=1024, pose="stereo"),
}
TILE, BOX_CAP = 16, 2048   # csrc/sweep_bwd_body.hpp: BT, BOX_CAP


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def atomic_bytes(d, s):
    """Bytes of float atomics of the g_src pass (see the module docstring)."""
    ix, iy = ops.sample_coords(d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], s["H"], s["W"], algo=_native.ALGO_DIRECT)
    H, W = s["H"], s["W"]
    big = 1 << 30
    total = 0
    for b in range(s["B"]):
        for v in range(s["V"]):
            x, y = ix[b, v], iy[b, v]            # [D,H,W]
            x0, y0 = torch.floor(x), torch.floor(y)
            fin = torch.isfinite(x) & torch.isfinite(y)
            xin0, xin1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
            yin0, yin1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
            anyx, anyy = (xin0 | xin1) & fin, (yin0 | yin1) & fin
            has = anyx & anyy
            xlo = torch.where(has, torch.where(xin0, x0, x0 + 1), torch.full_like(x, big))
            xhi = torch.where(has, torch.where(xin1, x0 + 1, x0), torch.full_like(x, -big))
            ylo = torch.where(has, torch.where(yin0, y0, y0 + 1), torch.full_like(y, big))
            yhi = torch.where(has, torch.where(yin1, y0 + 1, y0), torch.full_like(y, -big))
            taps = ((xin0.int() + xin1.int()) * (yin0.int() + yin1.int()) * fin.int())   # in-bounds taps per (plane, pixel)
            ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
            pad = lambda t, val: F.pad(t, (0, tx * TILE - W, 0, ty * TILE - H), value=val).reshape(-1, ty, TILE, tx, TILE)
            bx0 = pad(xlo, big).amin(dim=(2, 4))
            bx1 = pad(xhi, -big).amax(dim=(2, 4))
            by0 = pad(ylo, big).amin(dim=(2, 4))
            by1 = pad(yhi, -big).amax(dim=(2, 4))
            ntap = pad(taps.float(), 0).sum(dim=(2, 4))   # [D,ty,tx]
            D = bx0.shape[0]
            # greedy grouping of consecutive planes per tile, as the kernel does
            ux0 = torch.full((ty, tx), float(big), device=x.device)
            ux1, uy0, uy1 = -ux0.clone(), ux0.clone(), -ux0.clone()
            for k in range(D):
                nx0, nx1 = torch.minimum(ux0, bx0[k]), torch.maximum(ux1, bx1[k])
                ny0, ny1 = torch.minimum(uy0, by0[k]), torch.maximum(uy1, by1[k])
                na = torch.where(nx0 <= nx1, (nx1 - nx0 + 1) * (ny1 - ny0 + 1), torch.zeros_like(nx0))
                ua = torch.where(ux0 <= ux1, (ux1 - ux0 + 1) * (uy1 - uy0 + 1), torch.zeros_like(ux0))
                close = na > BOX_CAP                                 # flush the open group, start a new one at plane k
                total += float(ua[close].sum())
                single = torch.where(bx0[k] <= bx1[k], (bx1[k] - bx0[k] + 1) * (by1[k] - by0[k] + 1), torch.zeros_like(nx0))
                direct = close & (single > BOX_CAP)                   # the plane alone does not fit: its taps, directly
                total += float(ntap[k][direct].sum())
                ux0 = torch.where(close, torch.where(direct, float(big), bx0[k]), nx0)
                ux1 = torch.where(close, torch.where(direct, -float(big), bx1[k]), nx1)
                uy0 = torch.where(close, torch.where(direct, float(big), by0[k]), ny0)
                uy1 = torch.where(close, torch.where(direct, -float(big), by1[k]), ny1)
            total += float(torch.where(ux0 <= ux1, (ux1 - ux0 + 1) * (uy1 - uy0 + 1), torch.zeros_like(ux0)).sum())
    return int(total * s["C"] * 4)


def torch_sweep_chunks(ref, src, d, s, gcost, sigma, chunk):
    """The comparator: cost of planes [k, k + chunk) of view v, forward (and backward with gcost when it is given)."""
    B, V, C, H, W = src.shape
    dc = d["d_candi"]
    for i in range(B):
        for v in range(V):
            grid_all = O.plane_coords(d["K"][i], d["R"][i, v], d["t"][i, v], d["rays"][i], dc, d["cxcy"][i, 0], d["cxcy"][i, 1])
            for k0 in range(0, dc.numel(), chunk):
                n = min(chunk, dc.numel() - k0)
                grid = grid_all[k0:k0 + n].reshape(n, H, W, 2)
                warped = F.grid_sample(src[i, v].unsqueeze(0).expand(n, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                                       align_corners=False)
                cost = ((warped - ref[i].unsqueeze(0)) ** 2).sum(1) / sigma
                if gcost is not None:
                    (cost * gcost[i, k0:k0 + n]).sum().backward()


def bench_shape(name, s, reps, warmup, dev):
    b = synth.make_batch(77, s["B"], C=s["C"], D=s["D"], H=s["H"], W=s["W"], V=s["V"], pose=s["pose"])
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    d["d_candi"] = ops.d_candi_tensor(d["d_candi"], dev)
    sigma = 10.0
    ref = d["ref"].clone().requires_grad_(True)
    src = d["src"].clone().requires_grad_(True)
    gcost = torch.randn(s["B"], s["D"], s["H"], s["W"], device=dev)
    args = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], sigma)
    fwd = timed(lambda: ops.sweep_cost(ref, src, *args), reps, warmup)
    cost = ops.sweep_cost(ref, src, *args)
    bwd = timed(lambda: torch.autograd.backward(cost, gcost, retain_graph=True), reps, warmup)
    ref.grad = src.grad = None
    chunk = max(1, min(s["D"], (1 << 31) // (s["C"] * s["H"] * s["W"] * 4)))   # <= 2 GB of warped features per chunk
    treps = max(3, reps // 4)
    with torch.no_grad():
        tf = timed(lambda: torch_sweep_chunks(ref, src, d, s, None, sigma, chunk), treps, 1)
    tfb = timed(lambda: torch_sweep_chunks(ref, src, d, s, gcost, sigma, chunk), treps, 1)
    ref.grad = src.grad = None
    return dict(shape=s, fwd_ms=round(fwd, 4), bwd_ms=round(bwd, 4), torch_fwd_ms=round(tf, 3),
                torch_bwd_ms=round(tfb - tf, 3), torch_chunk_planes=chunk, atomic_bytes=atomic_bytes(d, s))


DET_SHAPES = {
    "model_step": dict(B=4, V=1, C=67, D=64, H=64, W=128, pose="mono"),
    "headline": SHAPES["headline"],
}


def bench_deterministic(s, reps, warmup, dev):
    import ctypes
    b = synth.make_batch(77, s["B"], C=s["C"], D=s["D"], H=s["H"], W=s["W"], V=s["V"], pose=s["pose"])
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    dc = ops.d_candi_tensor(d["d_candi"], dev)
    gcost = torch.randn(s["B"], s["D"], s["H"], s["W"], device=dev)
    args = (d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc, gcost, 10.0)
    run = {det: (lambda det=det: _native.sweep_backward(*args, want_ref=False, deterministic=det)[1]) for det in (False, True)}
    for _ in range(warmup):
        run[False](), run[True]()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(reps):
        for det in (False, True):   # the variants alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run[det]()
            e1.record()
            torch.cuda.synchronize()
            ms[det].append(e0.elapsed_time(e1))
    ga, gd = run[False](), run[True]()
    desc = _native.SweepDesc(s["B"], s["V"], s["C"], s["D"], s["H"], s["W"], 0, 1, 0, 10.0, 0, 0, 0)
    return dict(shape=s, atomic_ms=round(float(np.median(ms[False])), 4), det_ms=round(float(np.median(ms[True])), 4),
                workspace_bytes=int(_native.load().pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(desc))),
                max_rel_diff=float((ga - gd).abs().max() / ga.abs().max()), same_bits_twice=bool(torch.equal(gd, run[True]())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deterministic", action="store_true", help="time the g_src pass of the atomic and the deterministic path")
    ap.add_argument("--shapes", default="headline,training,config5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    if a.deterministic:
        for name, s in DET_SHAPES.items():
            out[name] = bench_deterministic(s, a.reps if a.reps != 20 else 50, a.warmup, dev)
        print(json.dumps(out))
        return
    for name in a.shapes.split(","):
        out[name] = bench_shape(name, SHAPES[name], a.reps, a.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
