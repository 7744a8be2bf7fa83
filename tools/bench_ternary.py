"""Time of the ternary census op (csrc/ternary.hip, ops.ternary) against the torch composition of the same formula (the patch as
K^2 shifted planes, then the elementwise chain over [B,K^2,H,W]; losses/loss_blocks.py:8-44 of the reference) on the same device and
inputs: forward alone, and forward plus backward with both gradients.

    python tools/bench_ternary.py [--shapes full,quarter] [--md 1,2,3] [--reps 25] [--warmup 5] [--rounds 2]

Prints ONE JSON line: per shape, md and direction the median over --reps x --rounds = 50 calls (device events around one call, after
--warmup calls; the two sides alternate --rounds times and the samples of all rounds are pooled) of hip_ms and composition_ms,
their ratio, and the algorithmic bytes of the op (forward 24 + 4 = 28 bytes per pixel, forward + backward 28 + 28 + 24 = 80) over
the HIP time.  Run the command twice for the spread between runs.  It gates nothing.
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
from pdepth_amd import ops  # noqa: E402

SHAPES = {"full": (4, 3, 256, 512), "quarter": (4, 3, 64, 128)}


def composition(x, y, md):
    k = 2 * md + 1
    H, W = x.shape[-2:]

    def transform(im):
        gray = ((im[:, 0] * 0.2989 + im[:, 1] * 0.5870 + im[:, 2] * 0.1140) * 255).unsqueeze(1)
        padded = F.pad(gray, [md] * 4)
        t = torch.cat([padded[:, :, dy:dy + H, dx:dx + W] for dy in range(k) for dx in range(k)], dim=1) - gray
        return t / torch.sqrt(0.81 + t * t)

    d = (transform(x) - transform(y)) ** 2
    mask = F.pad(x.new_ones(1, 1, H - 2 * md, W - 2 * md), [md] * 4)
    return (d / (0.1 + d)).mean(1, keepdim=True) * mask


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


def bench_shape(shape, md, reps, warmup, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(26)
    x = torch.rand(shape, generator=g, device=dev)
    y = (x + 0.05 * torch.randn(shape, generator=g, device=dev)).clamp(0, 1)
    B, _, H, W = shape
    g_out = torch.randn((B, 1, H, W), generator=g, device=dev)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def both(op):
        xg.grad = yg.grad = None
        op(xg, yg, md).backward(g_out)
        return xg.grad, yg.grad

    with torch.no_grad():   # the two sides compute the same thing
        assert float((ops.ternary(x, y, md) - composition(x, y, md)).abs().max()) <= 1e-4
    for a, b in zip(both(ops.ternary), both(composition)):
        assert float((a - b).abs().max()) <= 1e-2 * float(b.abs().max())
    sides = {"forward": {"hip_ms": lambda: ops.ternary(x, y, md), "composition_ms": lambda: composition(x, y, md)},
             "forward_backward": {"hip_ms": lambda: both(ops.ternary), "composition_ms": lambda: both(composition)}}
    pixels = B * H * W
    out = {"shape": list(shape), "md": md, "calls_per_side": reps * rounds}
    for direction, pair in sides.items():
        pooled = {k: [] for k in pair}
        with torch.set_grad_enabled(direction != "forward"):
            for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on both alike
                for k, fn in pair.items():
                    pooled[k] += timed(fn, reps, warmup)
        r = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
        r["composition_over_hip"] = round(r["composition_ms"] / r["hip_ms"], 2)
        nbytes = pixels * (28 if direction == "forward" else 28 + 52)
        r["hip_algorithmic_GBps"] = round(nbytes / (r["hip_ms"] * 1e-3) / 1e9, 1)
        out[direction] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="full,quarter")
    ap.add_argument("--md", default="1,2,3")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        for md in (int(m) for m in a.md.split(",")):
            out[f"{name}_md{md}"] = bench_shape(SHAPES[name], md, a.reps, a.warmup, a.rounds, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
