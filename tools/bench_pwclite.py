"""Time of the fused cost volume (csrc/cost_volume.hip: ops.flow_cost_volume, forward and forward plus backward) against the
composition of the ops it fuses (ops.flow_warp, ops.correlation, F.leaky_relu, autograd's backward), and of models.pwclite.PWCLite
forward plus backward through losses.flow_loss.unFlowLoss with fused_cost on and off -- same device, same inputs, one process.

    python tools/bench_pwclite.py [--cases l0,l1,l2,l3,l4,model] [--reps 25] [--warmup 10] [--rounds 2]

The op cases are PWCLite's five levels for a 384 x 832 input at B = 4: (C, h, w) = (192,6,13) (no flow), (128,12,26), (96,24,52),
(64,48,104), (32,96,208).  Prints ONE JSON line: per case the median over --reps x --rounds calls (device events around one call,
after --warmup calls; the sides alternate --rounds times and the samples of all rounds are pooled) of the fused side, of the
composition, and of the composition a second time (its ratio to the first is the run-to-run spread a ratio has to exceed to mean
anything), and the number of device kernels and memsets one call launches on each side (torch.profiler).  It gates nothing.
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import ops, synth  # noqa: E402
from pdepth_amd.losses.flow_loss import unFlowLoss  # noqa: E402
from pdepth_amd.models.pwclite import PWCLite  # noqa: E402
import util_cost_volume as U  # noqa: E402

LEVELS = {"l0": (192, 6, 13), "l1": (128, 12, 26), "l2": (96, 24, 52), "l3": (64, 48, 104), "l4": (32, 96, 208)}
B = 4


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


def launches(fn):
    """Device kernels and memsets / copies of one call, by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def composed(x1, x2, flow):
    warped = x2 if flow is None else ops.flow_warp(x2, flow, pad="border")
    return F.leaky_relu(ops.correlation(x1, warped, 4, 1, 4, 1, 1, 1), U.SLOPE)


def fused(x1, x2, flow):
    return ops.flow_cost_volume(x1, x2, flow, max_displacement=4, negative_slope=U.SLOPE, pad="border")


def level_case(name, dev):
    C, H, W = LEVELS[name]
    rs = np.random.RandomState(7)
    x1, x2 = (torch.from_numpy(rs.randn(B, C, H, W).astype(np.float32)).to(dev).requires_grad_(True) for _ in range(2))
    flow = None
    if name != "l0":
        coarse = torch.from_numpy(rs.randn(B, 2, 4, 6).astype(np.float32))
        flow = (2.0 * F.interpolate(coarse, (H, W), mode="bilinear", align_corners=True)).to(dev).contiguous().requires_grad_(True)
    go = torch.from_numpy(rs.randn(B, 81, H, W).astype(np.float32)).to(dev)
    wrt = (x1, x2) if flow is None else (x1, x2, flow)

    def fwd(op):
        with torch.no_grad():
            return op(x1, x2, flow)

    def both(op):
        return torch.autograd.grad(op(x1, x2, flow), wrt, go)
    a, b = both(fused), both(composed)
    agree = {"out_max": float((fwd(fused) - fwd(composed)).abs().max()), "grad_x1_max": float((a[0] - b[0]).abs().max()),
             "grad_x2_max": float((a[1] - b[1]).abs().max())}
    sides = {"forward": {"fused_ms": lambda: fwd(fused), "composition_ms": lambda: fwd(composed)},
             "forward_backward": {"fused_ms": lambda: both(fused), "composition_ms": lambda: both(composed)}}
    return sides, {"shape": [B, C, H, W], "flow": flow is not None, "difference": agree}


def model_case(dev):
    models = {}
    for key, on in (("fused_ms", True), ("composition_ms", False)):
        m = PWCLite(U.pwc_cfg(2, True), fused_cost=on)
        synth.seed_weights(m, seed=U.PWC_SEED, gain=U.PWC_GAIN)
        models[key] = m.to(dev)
    g = torch.Generator().manual_seed(11)
    wide = F.interpolate(torch.randn(B, 3, 24, 52, generator=g), (384 + 16, 832 + 16), mode="bicubic", align_corners=False)
    target = torch.cat([wide[:, :, 8:392, 8:840], wide[:, :, 6:390, 11:843]], 1).contiguous().to(dev)
    loss = unFlowLoss(U.train_cfg())

    def step(m):
        m.zero_grad(set_to_none=True)
        total = loss(U.train_output(m(target, with_bk=True)), target)[0]
        total.backward()
        return total
    totals = {k: float(step(m).detach()) for k, m in models.items()}
    return {"forward_backward": {k: (lambda m=m: step(m)) for k, m in models.items()}}, {"shape": [B, 6, 384, 832], "total": totals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="l0,l1,l2,l3,l4,model")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls_per_side": a.reps * a.rounds}
    for name in a.cases.split(","):
        groups, r = model_case(dev) if name == "model" else level_case(name, dev)
        for what, sides in groups.items():
            sides = dict(sides)
            sides["composition_again_ms"] = sides["composition_ms"]
            pooled = {k: [] for k in sides}
            for _ in range(a.rounds):   # the sides alternate: clock and thermal drift lands on all alike
                for k, fn in sides.items():
                    pooled[k] += timed(fn, a.reps, a.warmup)
            t = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
            t["composition_over_fused"] = round(t["composition_ms"] / t["fused_ms"], 2)
            t["spread"] = round(abs(t["composition_again_ms"] / t["composition_ms"] - 1.0), 3)
            t["launches"] = {"fused": launches(sides["fused_ms"]), "composition": launches(sides["composition_ms"])}
            r[what] = t
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
