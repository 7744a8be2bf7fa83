"""Time of the SSIM op (csrc/ssim.hip, ops.ssim) against the torch composition of the same formula (five average-pool passes and
the elementwise chain, losses/loss_blocks.py:47-66 of the reference) on the same device and inputs: forward alone, and forward
plus backward with both gradients.

    python tools/bench_ssim.py [--shapes full,quarter] [--md 1] [--reps 25] [--warmup 5] [--rounds 2]

Prints ONE JSON line: per shape and direction the median over --reps x --rounds = 50 calls (device events around one call, after --warmup calls;
the two sides alternate --rounds times and the samples of all rounds are pooled) of hip_ms and composition_ms, their ratio, and
the algorithmic bytes of the op (forward 12 bytes per element, forward + backward 12 + 20) over the HIP time.  Run the command
twice for the spread between runs.  It gates nothing.
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
from pdepth_amd import ops  # noqa: E402

SHAPES = {"full": (4, 3, 256, 512), "quarter": (4, 3, 64, 128)}
C1, C2 = 0.01 ** 2, 0.03 ** 2


def composition(x, y, md):
    pool = torch.nn.AvgPool2d(2 * md + 1, 1, 0)
    mx, my = pool(x), pool(y)
    mxy, mxx, myy = mx * my, mx.pow(2), my.pow(2)
    sx, sy, sxy = pool(x * x) - mxx, pool(y * y) - myy, pool(x * y) - mxy
    s = ((2 * mxy + C1) * (2 * sxy + C2)) / ((mxx + myy + C1) * (sx + sy + C2))
    return torch.clamp((1 - s) / 2, 0, 1)


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
    g = torch.Generator(device=dev).manual_seed(23)
    x = torch.rand(shape, generator=g, device=dev)
    y = (x + 0.05 * torch.randn(shape, generator=g, device=dev)).clamp(0, 1)
    B, C, H, W = shape
    g_out = torch.randn((B, C, H - 2 * md, W - 2 * md), generator=g, device=dev)
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def both(op):
        xg.grad = yg.grad = None
        op(xg, yg, md).backward(g_out)
        return xg.grad, yg.grad

    with torch.no_grad():   # the two sides compute the same thing
        assert float((ops.ssim(x, y, md) - composition(x, y, md)).abs().max()) <= 1e-5
    for a, b in zip(both(ops.ssim), both(composition)):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    sides = {"forward": {"hip_ms": lambda: ops.ssim(x, y, md), "composition_ms": lambda: composition(x, y, md)},
             "forward_backward": {"hip_ms": lambda: both(ops.ssim), "composition_ms": lambda: both(composition)}}
    elements = B * C * H * W
    out = {"shape": list(shape), "md": md, "calls_per_side": reps * rounds}
    for direction, pair in sides.items():
        pooled = {k: [] for k in pair}
        with torch.set_grad_enabled(direction != "forward"):
            for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on both alike
                for k, fn in pair.items():
                    pooled[k] += timed(fn, reps, warmup)
        r = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
        r["composition_over_hip"] = round(r["composition_ms"] / r["hip_ms"], 2)
        nbytes = elements * (12 if direction == "forward" else 32)
        r["hip_algorithmic_GBps"] = round(nbytes / (r["hip_ms"] * 1e-3) / 1e9, 1)
        out[direction] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="full,quarter")
    ap.add_argument("--md", type=int, default=1)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        out[name] = bench_shape(SHAPES[name], a.md, a.reps, a.warmup, a.rounds, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
