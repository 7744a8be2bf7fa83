"""Time of the fused photometric term of the flow loss (csrc/flow_photo.hip: ops.flow_photometric; unFlowLoss(cfg,
fused_photo=True)) against today's composition (ops.flow_warp, the mask products, ops.ssim, ops.ternary, the means and autograd's
backward), on the same device and inputs in one process, forward plus backward:

    photo_256x832, photo_128x416, photo_64x208   one level's photometric term alone at B = 4, weights (0.15, 0.85, 0.5)
    loss     unFlowLoss at DESIGN.md 6.11's configuration (B = 4, 256 x 832, three levels, occ_from_back, with_bk), switch on / off
    model    PWCLite + unFlowLoss, B = 4, 384 x 832 (DESIGN.md 6.12's row), switch on / off

    python tools/bench_flow_photo.py [--cases photo_256x832,photo_128x416,photo_64x208,loss,model] [--reps 25] [--warmup 10] [--rounds 2]

Prints ONE JSON line: per case the median over --reps x --rounds calls (device events around one call, after --warmup calls; the
sides alternate --rounds times and the samples of all rounds are pooled) of fused_ms, composition_ms and of the composition a second
time (composition_again_ms: its ratio to composition_ms is the run-to-run spread a ratio has to exceed to mean anything), and the
number of device kernels and memsets one call launches on each side (torch.profiler).  It gates nothing.
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
import util_cost_volume as UC  # noqa: E402
import util_flow as U  # noqa: E402
import util_flow_photo as P  # noqa: E402

B = 4
WEIGHTS = P.WEIGHTS[0]


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


def smooth_flow(rs, C, H, W, amp, dev):
    coarse = torch.from_numpy(rs.randn(B, C, 6, 9).astype(np.float32))
    return (amp * F.interpolate(coarse, (H, W), mode="bilinear", align_corners=True)).to(dev).contiguous()


def photo_case(H, W, dev):
    rs = np.random.RandomState(5)
    im, other = (torch.from_numpy(U.smooth_image(B, H, W, s)).to(dev) for s in (21, 22))
    flow = smooth_flow(rs, 2, H, W, 2.5, dev).requires_grad_(True)
    mask = (smooth_flow(rs, 1, H, W, 1.0, dev) > -0.8).float()
    composition = unFlowLoss(P.cfg_of(WEIGHTS))

    def fused():
        return torch.autograd.grad(ops.flow_photometric(im, other, flow, mask, *WEIGHTS)[0], flow)[0]

    def composed():
        return torch.autograd.grad(composition.loss_photomatric(im, ops.flow_warp(other, flow), mask), flow)[0]
    with torch.no_grad():
        values = (float(ops.flow_photometric(im, other, flow, mask, *WEIGHTS)[0]), float(composition.loss_photomatric(im, ops.flow_warp(other, flow), mask)))
    # (the flow's gradient jumps where a position crosses an integer: the median difference, next to the median gradient)
    agree = {"value": values, "grad_median_difference": float((fused() - composed()).abs().median()), "grad_median": float(composed().abs().median())}
    return {"fused_ms": fused, "composition_ms": composed}, {"shape": [B, H, W], "seen": round(float(mask.mean()), 3), "agreement": agree}


def loss_case(dev, H=256, W=832):
    rs = np.random.RandomState(3)
    target = torch.cat((torch.from_numpy(U.smooth_image(B, H, W, 11)), torch.from_numpy(U.smooth_image(B, H, W, 12))), 1).to(dev)
    flows = []
    for i in range(3):
        h, w = H >> i, W >> i
        fwd = smooth_flow(rs, 2, h, w, 2.5 / 2 ** i, dev)
        flows.append(torch.cat((fwd, -fwd + smooth_flow(rs, 2, h, w, 0.5 / 2 ** i, dev)), 1).requires_grad_(True))
    sides, totals = {}, {}
    for key, on in (("fused_ms", True), ("composition_ms", False)):
        loss = unFlowLoss(U.unflow_cfg(True, True, "border"), fused_photo=on)
        sides[key] = lambda loss=loss: torch.autograd.grad(loss(flows, target)[0], flows)
        totals[key[:-3]] = float(loss(flows, target)[0].detach())
    return sides, {"shape": [B, 4, H, W], "levels": 3, "total": totals}


def model_case(dev):
    model = PWCLite(UC.pwc_cfg(2, True)).to(dev)
    synth.seed_weights(model, seed=UC.PWC_SEED, gain=UC.PWC_GAIN)
    g = torch.Generator().manual_seed(11)
    wide = F.interpolate(torch.randn(B, 3, 24, 52, generator=g), (384 + 16, 832 + 16), mode="bicubic", align_corners=False)
    target = torch.cat([wide[:, :, 8:392, 8:840], wide[:, :, 6:390, 11:843]], 1).contiguous().to(dev)
    sides, totals = {}, {}
    for key, on in (("fused_ms", True), ("composition_ms", False)):
        loss = unFlowLoss(UC.train_cfg(), fused_photo=on)

        def step(loss=loss):
            model.zero_grad(set_to_none=True)
            total = loss(UC.train_output(model(target, with_bk=True)), target)[0]
            total.backward()
            return total
        sides[key] = step
        totals[key[:-3]] = float(step().detach())
    return sides, {"shape": [B, 6, 384, 832], "total": totals}


CASES = {"photo_256x832": lambda dev: photo_case(256, 832, dev), "photo_128x416": lambda dev: photo_case(128, 416, dev),
         "photo_64x208": lambda dev: photo_case(64, 208, dev), "loss": loss_case, "model": model_case}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
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
        r["composition_over_fused"] = round(r["composition_ms"] / r["fused_ms"], 2)
        r["spread"] = round(abs(r["composition_again_ms"] / r["composition_ms"] - 1.0), 3)
        r["launches"] = {"fused": launches(sides["fused_ms"]), "composition": launches(sides["composition_ms"])}
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
