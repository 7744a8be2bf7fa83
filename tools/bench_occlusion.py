"""Time of the occlusion-mask ops (csrc/occlusion.hip: ops.depth_occlusion, ops.occlusion_mask) against the torch composition of the
same computation on the same device and inputs: tests/util_occlusion.py in float32 -- the depth-to-position chain with two batched
matmuls, then the four-tap splat with scatter_add_ and the threshold.

    python tools/bench_occlusion.py [--shapes full,quarter] [--reps 25] [--warmup 10] [--rounds 2]

Prints ONE JSON line: per shape and op the median over --reps x --rounds = 50 calls (device events around one call, after --warmup
calls; the two sides alternate --rounds times and the samples of all rounds are pooled) of hip_ms and composition_ms and their
ratio.  The scene is the tests' box on a slanted background, so that destinations collide as they do in use.  Run the command twice
for the spread between runs.  It gates nothing.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import ops  # noqa: E402
import util_occlusion as U  # noqa: E402

SHAPES = {"full": (4, 256, 512), "quarter": (4, 64, 128)}
TH = 0.2


def scene(shape, dev):
    """A 5 m box on an 18-25 m slanted background, a camera 0.54 m to the side with a yaw of 2 degrees, f = 0.75 W."""
    B, H, W = shape
    f = 0.75 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.stack([18.0 + 7.0 * (xs / (W - 1.0) if b % 2 == 0 else 1 - xs / (W - 1.0)) + 0.3 * ys / (H - 1.0) for b in range(B)])
    for b in range(B):
        depth[b, H // 4 + 3 * b:H // 4 + 3 * b + H // 3, W // 4 + 5 * b:W // 4 + 5 * b + W // 4] = 5.0
    a = np.deg2rad(2.0)
    pose = np.eye(4)
    pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    pose[:3, 3] = [0.54, 0.0, -0.3]

    def t(m):
        return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m, (B,) + m.shape), dtype=np.float32)).to(dev)
    return torch.from_numpy(depth.astype(np.float32)).to(dev), t(np.linalg.inv(K)), t(K @ pose[:3])


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
    depth, Kinv, proj = scene(shape, dev)
    coords = U.depth_positions(depth, Kinv, proj).contiguous()
    sides = {"depth_occlusion": {"hip_ms": lambda: ops.depth_occlusion(depth, Kinv, proj, TH),
                                 "composition_ms": lambda: U.visible(U.range_map(U.depth_positions(depth, Kinv, proj)), TH)},
             "occlusion_mask": {"hip_ms": lambda: ops.occlusion_mask(coords, TH),
                                "composition_ms": lambda: U.visible(U.range_map(coords), TH)}}
    out = {"shape": list(shape), "calls_per_side": reps * rounds}
    with torch.no_grad():
        for op, pair in sides.items():
            a, b = pair["hip_ms"](), pair["composition_ms"]()   # the two sides compute the same thing
            differ = float((a != b).float().mean())
            assert differ <= 1e-3, (op, differ)
            pooled = {k: [] for k in pair}
            for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on both alike
                for k, fn in pair.items():
                    pooled[k] += timed(fn, reps, warmup)
            r = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
            r["composition_over_hip"] = round(r["composition_ms"] / r["hip_ms"], 2)
            r["occluded_share"] = round(1.0 - float(a.mean()), 4)
            r["mask_pixels_that_differ"] = differ
            out[op] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="full,quarter")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        out[name] = bench_shape(SHAPES[name], a.reps, a.warmup, a.rounds, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
