"""Time of the device-side depth metrics (ops.depth_metrics: csrc/metrics.hip) against the expectation kernel that reads the
same bytes, and against the read-back path it replaces.

    python tools/bench_metrics.py [--shapes refined] [--reps 20] [--warmup 3] [--rounds 3]

Prints ONE JSON line: per shape the median over --reps calls (device events, after --warmup calls; the sides alternate --rounds
times and the samples of all rounds are pooled) of
  volume_ms       : ops.depth_metrics(truth, logp=..., mask, clamp_max): expectation + nine errors from one read of the volume;
  volume_depth_ms : the same with want_depth (the depth map written from the same pass);
  expect_ms       : ops.dpv_expect on the same volume, the yardstick: the kernel that reads the same bytes and only writes the map;
  map_ms          : ops.depth_metrics(truth, pred=...) on the depth map ops.dpv_expect left behind;
  host_ms         : the path replaced, per batch: clamp + mask on the device, both maps of every item copied to the host, the nine
                    errors with numpy (wall clock, the expectation not included);
  volume_gbs / expect_gbs : the bytes each must move over its time.
It gates nothing.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import ops, synth  # noqa: E402

SHAPES = {"lowres": (4, 64, 64, 128), "refined": (4, 64, 256, 512)}


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


def timed_wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def numpy_errors(p, t):
    """The nine errors of one item on the host (float64 numpy; the devkit's loop is C++ and not part of this repository)."""
    p = np.where(p == 0, -1.0, p).astype(np.float64)
    t = np.where(t == 0, -1.0, t).astype(np.float64)
    v = p >= 0
    p, t, n = p[v], t[v], int(v.sum())
    e, ei, s = np.abs(p - t), np.abs(1 / p - 1 / t), np.log(p) - np.log(t)
    sq = (s * s).sum() / n
    return [e.sum() / n, np.sqrt((e * e).sum() / n), ei.sum() / n, np.sqrt((ei * ei).sum() / n), np.abs(s).sum() / n, np.sqrt(sq),
            np.sqrt(sq - s.sum() ** 2 / n ** 2), (e / p).sum() / n, (e * e / (p * p)).sum() / n]


def bench_shape(shape, reps, warmup, rounds, dev):
    B, D, H, W = shape
    g = torch.Generator(device=dev).manual_seed(5)
    logp = torch.log_softmax(2 * torch.randn(shape, generator=g, device=dev), 1)
    dcl = synth.powerf(5.0, 40.0, D, 1.0)
    dc = ops.d_candi_tensor(dcl, dev)
    clamp = float(dcl[-1])
    depth = ops.dpv_expect(logp, dc, BV_log=True)
    mask = (torch.rand(B, 1, H, W, generator=g, device=dev) < 0.6).float()
    truth = depth * torch.exp(0.3 * torch.randn(B, H, W, generator=g, device=dev)) * mask[:, 0]

    def host():
        t = truth.clone()
        t[t >= clamp] = clamp
        p = depth * mask[:, 0]
        return [numpy_errors(p[b].cpu().numpy(), t[b].cpu().numpy()) for b in range(B)]

    sides = {"volume_ms": lambda: ops.depth_metrics(truth, logp=logp, d_candi=dc, mask=mask, clamp_max=clamp),
             "volume_depth_ms": lambda: ops.depth_metrics(truth, logp=logp, d_candi=dc, mask=mask, clamp_max=clamp, want_depth=True),
             "expect_ms": lambda: ops.dpv_expect(logp, dc, BV_log=True),
             "map_ms": lambda: ops.depth_metrics(truth, pred=depth, mask=mask, clamp_max=clamp)}
    got = ops.depth_metrics(truth, logp=logp, d_candi=dc, mask=mask, clamp_max=clamp)[0].cpu().numpy()
    np.testing.assert_allclose(got, np.asarray(host()), rtol=1e-5)
    pooled = {k: [] for k in list(sides) + ["host_ms"]}
    with torch.no_grad():
        for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on all of them alike
            for k, fn in sides.items():
                pooled[k] += timed(fn, reps, warmup)
            pooled["host_ms"] += timed_wall(host, max(reps // 4, 3), 1)
    out = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
    vol, px = 4.0 * B * D * H * W, 4.0 * B * H * W
    out["volume_gbs"] = round((vol + 2 * px) / out["volume_ms"] / 1e6, 1)
    out["expect_gbs"] = round((vol + px) / out["expect_ms"] / 1e6, 1)
    out["volume_over_expect"] = round(out["volume_ms"] / out["expect_ms"], 3)
    out["shape"] = list(shape)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="refined")
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
