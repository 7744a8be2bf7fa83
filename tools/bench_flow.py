"""Time of the flow-loss ops (csrc/flow_warp.hip, csrc/loss_smooth1.hip: ops.flow_warp with its backward, ops.flow_fb_check, and
losses.flow_loss.unFlowLoss over them) against the torch compositions they replace, on the same device and inputs in one process:
flow_warp as mesh grid, normalisation and F.grid_sample with autograd's backward; get_occu_mask_bidirection over that; unFlowLoss
with those two and the torch smooth_grad_1st (tests/util_flow.smooth_ref) in place of the three ops, everything else (SSIM, census,
range map) the same HIP ops on both sides.

    python tools/bench_flow.py [--cases warp_c3,warp_c192,fb,loss] [--reps 25] [--warmup 10] [--rounds 2]

Prints ONE JSON line: per case the median over --reps x --rounds calls (device events around one call, after --warmup calls; the
sides alternate --rounds times and the samples of all rounds are pooled) of hip_ms, composition_ms and of the composition a second
time (composition_again_ms: its ratio to composition_ms is the run-to-run spread a ratio has to exceed to mean anything), and the
number of device kernels and memsets one call launches on each side (torch.profiler).  It gates nothing.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import ops  # noqa: E402
from pdepth_amd.losses import flow_loss  # noqa: E402
import util_flow as U  # noqa: E402


def compose_flow_warp(x, flow12, pad="border"):
    """The torch composition: base grid + flow, 2 v / (W - 1) - 1, F.grid_sample(align_corners=False)."""
    B, _, H, W = x.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack((xs, ys), 0).unsqueeze(0).repeat(B, 1, 1, 1).to(device=x.device, dtype=x.dtype)
    v = base + flow12
    grid = torch.stack((2.0 * v[:, 0] / (W - 1) - 1.0, 2.0 * v[:, 1] / (H - 1) - 1.0), -1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode=pad, align_corners=False)


def compose_fb_check(flow12, flow21, scale=0.01, bias=0.5):
    back = compose_flow_warp(flow21, flow12, pad="zeros")
    both = flow12 + back
    mag = (flow12 * flow12).sum(1, keepdim=True) + (back * back).sum(1, keepdim=True)
    return ((both * both).sum(1, keepdim=True) > scale * mag + bias).float()


_COMPOSED = types.SimpleNamespace(flow_warp=compose_flow_warp, smooth_grad_1st=U.smooth_ref, ssim=ops.ssim, ternary=ops.ternary,
                                  flow_fb_check=lambda a, b: compose_fb_check(a.detach(), b.detach()))


def composed_loss(loss, flows, target):
    """unFlowLoss with the three new ops replaced by their torch compositions."""
    flow_loss.ops = _COMPOSED
    try:
        return loss(flows, target)
    finally:
        flow_loss.ops = ops


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


def smooth_flow(rs, B, C, H, W, amp, dev):
    coarse = torch.from_numpy(rs.randn(B, C, 6, 9).astype(np.float32))
    return (amp * F.interpolate(coarse, (H, W), mode="bilinear", align_corners=True)).to(dev).contiguous()


def warp_case(B, C, H, W, dev):
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randn(B, C, H, W).astype(np.float32)).to(dev).requires_grad_(True)
    flow = smooth_flow(rs, B, 2, H, W, 3.0 if H > 16 else 1.0, dev).requires_grad_(True)
    go = torch.from_numpy(rs.randn(B, C, H, W).astype(np.float32)).to(dev)

    def run(warp):
        return torch.autograd.grad(warp(x, flow, pad="border"), (x, flow), go)
    a, b = run(ops.flow_warp), run(compose_flow_warp)   # the two sides compute the same thing
    with torch.no_grad():
        d_out = float((ops.flow_warp(x, flow, pad="border") - compose_flow_warp(x, flow, pad="border")).abs().max())
    # (the flow's gradient jumps where a position crosses an integer, and the two sides round positions differently: its median)
    agree = {"out_max": d_out, "grad_x_max": float((a[0] - b[0]).abs().max()), "grad_flow_median": float((a[1] - b[1]).abs().median())}
    return {"hip_ms": lambda: run(ops.flow_warp), "composition_ms": lambda: run(compose_flow_warp)}, {"shape": [B, C, H, W],
                                                                                                    "difference": agree}


def fb_case(B, H, W, dev):
    rs = np.random.RandomState(2)
    f12 = smooth_flow(rs, B, 2, H, W, 3.0, dev)
    f21 = (-f12 + 0.6 * torch.from_numpy(rs.randn(B, 2, H, W).astype(np.float32)).to(dev)).contiguous()
    differ = float((ops.flow_fb_check(f12, f21) != compose_fb_check(f12, f21)).float().mean())
    return {"hip_ms": lambda: ops.flow_fb_check(f12, f21), "composition_ms": lambda: compose_fb_check(f12, f21)}, {
        "shape": [B, 2, H, W], "mask_pixels_that_differ": differ}


def loss_case(B, H, W, dev):
    rs = np.random.RandomState(3)
    target = torch.cat((torch.from_numpy(U.smooth_image(B, H, W, 11)), torch.from_numpy(U.smooth_image(B, H, W, 12))), 1).to(dev)
    flows = []
    for i in range(3):
        h, w = H >> i, W >> i
        fwd = smooth_flow(rs, B, 2, h, w, 2.5 / 2 ** i, dev)
        flows.append(torch.cat((fwd, -fwd + smooth_flow(rs, B, 2, h, w, 0.5 / 2 ** i, dev)), 1).requires_grad_(True))
    loss = flow_loss.unFlowLoss(U.unflow_cfg(True, True, "border"))

    def run(call):
        return torch.autograd.grad(call()[0], flows)
    hip, comp = (lambda: run(lambda: loss(flows, target))), (lambda: run(lambda: composed_loss(loss, flows, target)))
    total = (float(loss(flows, target)[0].detach()), float(composed_loss(loss, flows, target)[0].detach()))
    return {"hip_ms": hip, "composition_ms": comp}, {"shape": [B, 4, H, W], "levels": 3, "total": total}


CASES = {"warp_c3": lambda dev: warp_case(4, 3, 256, 832, dev), "warp_c192": lambda dev: warp_case(4, 192, 4, 8, dev),
         "fb": lambda dev: fb_case(4, 256, 832, dev), "loss": lambda dev: loss_case(4, 256, 832, dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="warp_c3,warp_c192,fb,loss")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "calls_per_side": a.reps * a.rounds}
    for name in a.cases.split(","):
        sides, r = CASES[name](dev)
        sides["composition_again_ms"] = sides["composition_ms"]
        pooled = {k: [] for k in sides}
        for _ in range(a.rounds):   # the sides alternate: clock and thermal drift lands on all alike
            for k, fn in sides.items():
                pooled[k] += timed(fn, a.reps, a.warmup)
        r.update({k: round(float(np.median(v)), 4) for k, v in pooled.items()})
        r["composition_over_hip"] = round(r["composition_ms"] / r["hip_ms"], 2)
        r["spread"] = round(abs(r["composition_again_ms"] / r["composition_ms"] - 1.0), 3)
        r["launches"] = {"hip": launches(sides["hip_ms"]), "composition": launches(sides["composition_ms"])}
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
