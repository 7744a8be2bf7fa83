"""Time of the fused photometric term (csrc/photo.hip, ops.rgb_stereo_consistency(..., ssim_weight=0.85)) against the composition it
replaces, loss_blocks.rgb_stereo_consistency_loss(..., ssim_weight=0.85, per_item=True) with fused=False -- the HIP warp, the torch
elementwise passes and masked means, the HIP SSIM, and autograd's replay of all of it --, on the same device and inputs: forward
alone, and forward plus backward down to the gradient of the depth map.

    python tools/bench_photo.py [--shapes full,quarter] [--md 1] [--reps 25] [--warmup 5] [--rounds 2]

Prints ONE JSON line: per shape and direction the median over --reps x --rounds = 50 calls (device events around one call, after
--warmup calls; the sides alternate --rounds times and the samples of all rounds are pooled) of
    op_ms            ops.rgb_stereo_consistency with the camera matrices given, as BaseLoss(fused_photo=True) calls it,
    function_ms      loss_blocks.rgb_stereo_consistency_loss(..., fused=True): the same op behind the matrices' formation,
    composition_ms   the same function with fused=False,
the ratios composition / op and composition / function, and the algorithmic bytes of the op (forward 4 (1 + 3) read + 48 gathered per
pixel, forward + backward twice that + 4 written) over op_ms.  Run the command twice for the spread between runs.  It gates nothing.
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
from pdepth_amd.losses import loss_blocks as lb  # noqa: E402

SHAPES = {"full": (4, 3, 256, 512), "quarter": (4, 3, 64, 128)}
W_SSIM = 0.85


def make_inputs(shape, dev):
    """A stereo pair's worth of inputs: images in [0, 1] that share their coarse structure, a smooth depth map of 8 to 36 m, a
    0.54 m baseline, intrinsics scaled to the image."""
    B, _, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(29)
    up = lambda t: torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=True)
    base = up(torch.rand(B, 3, H // 4, W // 4, generator=g))
    src = 0.8 * base + 0.2 * torch.rand(B, 3, H, W, generator=g)
    tgt = 0.8 * base + 0.2 * torch.rand(B, 3, H, W, generator=g)
    depth = up(9.0 + 26.0 * torch.rand(B, 1, H // 8, W // 8, generator=g))[:, 0] + torch.rand(B, H, W, generator=g) - 0.5
    K = torch.tensor([[0.85 * W, 0.0, 0.5 * W], [0.0, 1.1 * H, 0.49 * H], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([-0.54, 0.01, 0.0])
    return tuple(t.float().to(dev).contiguous() for t in (src, tgt, depth, K, pose.unsqueeze(0)))


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
    src, tgt, depth, K, pose = make_inputs(shape, dev)
    B, _, H, W = shape
    Kinv, proj = lb._inv3(K).expand(B, 3, 3).contiguous(), torch.matmul(K, pose[:, 0:3, :]).expand(B, 3, 4).contiguous()
    g_value = torch.arange(1, B + 1, dtype=torch.float32, device=dev)
    leaf = depth.clone().requires_grad_(True)
    photo = {"ssim_weight": W_SSIM, "ssim_md": md}
    sides = {"op_ms": lambda d: ops.rgb_stereo_consistency(src, tgt, d, Kinv, proj, **photo)[0],
             "function_ms": lambda d: lb.rgb_stereo_consistency_loss(src, tgt, d, pose, K, per_item=True, fused=True, **photo),
             "composition_ms": lambda d: lb.rgb_stereo_consistency_loss(src, tgt, d, pose, K, per_item=True, **photo)}

    def both(fn):
        leaf.grad = None
        fn(leaf).backward(g_value)
        return leaf.grad

    with torch.no_grad():   # the sides compute the same thing
        values = {k: fn(depth) for k, fn in sides.items()}
    grads = {k: both(fn) for k, fn in sides.items()}
    for k in ("op_ms", "function_ms"):
        assert float((values[k] - values["composition_ms"]).abs().max()) <= 1e-5 * float(values["composition_ms"].abs().max())
        assert float((grads[k] - grads["composition_ms"]).abs().max()) <= 1e-4 * float(grads["composition_ms"].abs().max())
    out = {"shape": list(shape), "md": md, "calls_per_side": reps * rounds, "mask_pixels_per_item": None}
    with torch.no_grad():
        out["mask_pixels_per_item"] = ops.rgb_stereo_consistency(src, tgt, depth, Kinv, proj, **photo)[1].tolist()
    pixels = B * H * W
    for direction in ("forward", "forward_backward"):
        pooled = {k: [] for k in sides}
        with torch.set_grad_enabled(direction != "forward"):
            for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on all alike
                for k, fn in sides.items():
                    call = (lambda fn=fn: fn(depth)) if direction == "forward" else (lambda fn=fn: both(fn))
                    pooled[k] += timed(call, reps, warmup)
        r = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
        r["composition_over_op"] = round(r["composition_ms"] / r["op_ms"], 2)
        r["composition_over_function"] = round(r["composition_ms"] / r["function_ms"], 2)
        nbytes = pixels * (64 if direction == "forward" else 2 * 64 + 4)
        r["op_algorithmic_GBps"] = round(nbytes / (r["op_ms"] * 1e-3) / 1e9, 1)
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
