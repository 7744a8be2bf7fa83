"""Forward + backward time of the fused soft-label cross-entropy + depth (ops.dpv_soft_ce: csrc/loss.hip) against the same
formula in PyTorch ops on the same device.

    python tools/bench_loss.py [--shapes lowres,refined,config5] [--reps 20] [--warmup 3] [--rounds 3]

Prints ONE JSON line: per shape the median over --reps forward+backward calls (device events, after --warmup calls; the two
sides alternate --rounds times and the medians of all rounds are pooled) of
  label_ms / from_depth_ms : loss and depth of ops.dpv_soft_ce with a label tensor / with the label formed from a depth map,
                             then backward of loss.sum() + (depth * g).sum();
  torch_ms                 : the comparator: -(label * logp).sum(1) masked mean per item and (d_candi * exp(logp)).sum(1), autograd;
  reduce_ms                : ops.dpv_reduce on the same shape (reads and writes the volume once), the streaming yardstick;
  label_gbs / from_depth_gbs / reduce_gbs : the bytes each must move (see csrc/loss.hip) over its time.
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
from pdepth_amd import ops, synth  # noqa: E402

SHAPES = {"lowres": (4, 64, 64, 96), "refined": (4, 64, 256, 384), "config5": (2, 128, 512, 1024)}


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


def bench_shape(shape, reps, warmup, rounds, dev):
    B, D, H, W = shape
    g = torch.Generator(device=dev).manual_seed(5)
    logp = torch.log_softmax(2 * torch.randn(shape, generator=g, device=dev), 1)
    label = torch.softmax(3 * torch.randn(shape, generator=g, device=dev), 1)
    mask = (torch.rand(B, H, W, generator=g, device=dev) < 0.6).float()
    depth_gt = 5.0 + 35.0 * torch.rand(B, H, W, generator=g, device=dev)
    gd = torch.randn(B, H, W, generator=g, device=dev)
    dc = ops.d_candi_tensor(synth.powerf(5.0, 40.0, D, 1.0), dev)
    x = logp.clone().requires_grad_(True)

    def fused(**src):
        x.grad = None
        loss, depth = ops.dpv_soft_ce(x, dc, mask=mask, want_depth=True, **src)
        (loss.sum() + (depth * gd).sum()).backward()

    def composed():
        x.grad = None
        ce = -(label * x).sum(1) * mask
        cnt = (mask == 1).sum((1, 2))
        loss = torch.where(cnt > 0, ce.sum((1, 2)) / cnt.clamp(min=1), torch.zeros_like(cnt, dtype=torch.float32))
        depth = (dc.view(1, D, 1, 1) * torch.exp(x)).sum(1)
        (loss.sum() + (depth * gd).sum()).backward()

    def reduce():
        with torch.no_grad():
            ops.dpv_reduce(logp, dc)

    sides = {"label_ms": lambda: fused(label=label), "from_depth_ms": lambda: fused(depth_gt=depth_gt, variance=0.3),
             "torch_ms": composed, "reduce_ms": reduce}
    pooled = {k: [] for k in sides}
    for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on all of them alike
        for k, fn in sides.items():
            pooled[k] += timed(fn, reps, warmup)
    out = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
    vol, px = 4.0 * B * D * H * W, 4.0 * B * H * W
    moved = {"label": 2 * vol + 2 * px + 2 * vol + vol + 2 * px, "from_depth": vol + 3 * px + 2 * vol + 3 * px, "reduce": 2 * vol + px}
    for k, nbytes in moved.items():
        out[k + "_gbs"] = round(nbytes / out[k + "_ms"] / 1e6, 1)
    out["shape"] = list(shape)
    out["speedup_label"] = round(out["torch_ms"] / out["label_ms"], 2)
    out["speedup_from_depth"] = round(out["torch_ms"] / out["from_depth_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="lowres,refined,config5")
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
