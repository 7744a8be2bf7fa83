"""Time of the DPV fusion backward (csrc/dpv_fuse_bwd.hip behind ops.dpv_fuse) against the backward of the torch composition it
replaces and against the fusion forward, the bandwidth yardstick.

    python tools/bench_fuse_backward.py [--shapes lowres,refined] [--reps 20] [--warmup 3] [--rounds 3]

Prints ONE JSON line: per shape the median over --reps x --rounds calls (device events, after --warmup calls; the sides alternate
--rounds times and the samples of all rounds are pooled) of
  hip_bwd_ms   : the HIP backward with both incoming gradients present (reads 3 V + 2 P, writes V);
  torch_bwd_ms : autograd's backward through the float32 torch composition of models/models.py:666-672 with
                 utils/img_utils.py:31-47, :360-375 on the same device (the graph is recorded once, outside the clock);
  fwd_ms       : ops.dpv_fuse forward with both outputs on the same volume (reads V + 2 P, writes 2 V);
  hip_bwd_tbs / fwd_tbs : the bytes each must move over its time, V = 4 B D H W, P = 4 B H W.
It gates nothing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import _native, ops, synth  # noqa: E402

SHAPES = {"lowres": (4, 64, 64, 128), "refined": (4, 64, 256, 512)}
VAR, EPS = 0.3, torch.finfo(float).eps


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
    return ms


def fuse_torch(logp, dmaps, masks, dc):
    d = dc.view(1, -1, 1, 1)
    sigma = torch.sqrt(torch.tensor(VAR, device=logp.device))
    dists = torch.exp(-torch.pow(torch.abs(d - dmaps.unsqueeze(1)), 2.0) / (2 * torch.pow(sigma, 2.0)))
    dists = dists / torch.sum(dists, dim=1, keepdim=True)
    dists = torch.where(dists != dists, torch.full_like(dists, -1.0), dists)
    mask = masks.unsqueeze(1)
    tofuse = torch.clamp(dists * mask + (1.0 / d.shape[1]) * (1.0 - mask), EPS, 1.0)
    fused = torch.exp(logp + torch.log(tofuse))
    fused = torch.clamp(fused / torch.sum(fused, dim=1, keepdim=True), EPS, 1.0)
    return fused, torch.log(fused)


def bench_shape(shape, reps, warmup, rounds, dev):
    B, D, H, W = shape
    g = torch.Generator(device=dev).manual_seed(5)
    logp = torch.log_softmax(3 * torch.randn(shape, generator=g, device=dev), 1)
    dc = ops.d_candi_tensor(synth.powerf(5.0, 40.0, D, 1.0), dev)
    dmaps = 3 + 39 * torch.rand(B, H, W, generator=g, device=dev)
    masks = (torch.rand(B, H, W, generator=g, device=dev) < 0.5).float()
    g_f = torch.randn(shape, generator=g, device=dev)
    g_l = torch.randn(shape, generator=g, device=dev)

    x = logp.clone().requires_grad_(True)
    fused, logf = fuse_torch(x, dmaps, masks, dc)
    sides = {"hip_bwd_ms": lambda: _native.dpv_fuse_backward(logp, dmaps, masks, dc, VAR, EPS, g_f, g_l),
             "torch_bwd_ms": lambda: torch.autograd.grad((fused, logf), x, (g_f, g_l), retain_graph=True),
             "fwd_ms": lambda: ops.dpv_fuse(logp, dmaps, masks, dc, var=VAR)}
    hip, ref = sides["hip_bwd_ms"](), sides["torch_bwd_ms"]()[0]
    diff = float((hip - ref).abs().median() / ref.abs().max())   # (the median: a plane on the clamp boundary may flip)
    assert diff <= 1e-5, diff
    pooled = {k: [] for k in sides}
    for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on all of them alike
        for k, fn in sides.items():
            pooled[k] += timed(fn, reps, warmup)
    out = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
    vol, px = 4.0 * B * D * H * W, 4.0 * B * H * W
    out["hip_bwd_tbs"] = round((4 * vol + 2 * px) / out["hip_bwd_ms"] / 1e9, 3)
    out["fwd_tbs"] = round((3 * vol + 2 * px) / out["fwd_ms"] / 1e9, 3)
    out["torch_over_hip"] = round(out["torch_bwd_ms"] / out["hip_bwd_ms"], 2)
    out["calls_per_side"] = reps * rounds
    out["shape"] = list(shape)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lowres,refined")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        out[name] = bench_shape(SHAPES[name], a.reps, a.warmup, a.rounds, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
