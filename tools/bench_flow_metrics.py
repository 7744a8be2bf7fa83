"""Time of the device-side flow evaluation (ops.flow_metrics, ops.flow_resize: csrc/flow_metrics.hip) against the path a user
has without it.

    python tools/bench_flow_metrics.py [--shapes sintel,kitti] [--reps 20] [--warmup 3] [--rounds 3]

Prints ONE JSON line: per shape (B = 4, prediction 384 x 832; sintel: 2-channel truth 436 x 1024; kitti: 4-channel truth
375 x 1242 with a move mask) the median over --reps calls (device events, after --warmup calls; the sides alternate --rounds
times and the samples of all rounds are pooled) of
  metrics_ms      : ops.flow_metrics(gt, pred[, move_mask]): rescale, resize, end-point error, sums, two launches;
  metrics_flow_ms : the same with want_flow (the resized flow written from the same pass);
  resize_ms       : ops.flow_resize(pred, (H, W)) alone;
  host_ms         : the path without it, per batch: the prediction copied to the host, numpy's rescale, a numpy bilinear resize
                    (OpenCV's rule; OpenCV itself is not a dependency of this package), the per-item loop of
                    utils/flow_utils.evaluate_flow restated in numpy (wall clock, the truth already on the host);
  metrics_gbs     : the bytes ops.flow_metrics must move (truth, masks, prediction once) over its time.
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
from pdepth_amd import ops  # noqa: E402

# name -> (B, (h, w), (H, W), channels of the truth, move mask)
SHAPES = {"sintel": (4, (384, 832), (436, 1024), 2, False), "kitti": (4, (384, 832), (375, 1242), 4, True)}


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


def _axis(n_out, n_in):
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(s).astype(np.int64)
    f = (s - i0).astype(np.float32)
    f[i0 < 0] = 0
    i0[i0 < 0] = 0
    f[i0 >= n_in - 1] = 0
    i0[i0 >= n_in - 1] = n_in - 1
    return i0, np.minimum(i0 + 1, n_in - 1), f


def numpy_resize(src, H, W):
    """[h,w,C] float32 -> [H,W,C]: OpenCV's INTER_LINEAR rule in numpy."""
    (y0, y1, fy), (x0, x1, fx) = _axis(H, src.shape[0]), _axis(W, src.shape[1])
    fx, fy = fx.reshape(1, W, 1), fy.reshape(H, 1, 1)
    rows = src[:, x0] * (1 - fx) + src[:, x1] * fx
    return rows[y0] * (1 - fy) + rows[y1] * fy


def numpy_evaluate(gts, pred_dev, moves):
    """evaluate_flow's loop (utils/flow_utils.py:61-123) in numpy, the prediction read back first."""
    preds = pred_dev.cpu().numpy().transpose(0, 2, 3, 1)
    rows = []
    for i, (gt, pred) in enumerate(zip(gts, preds)):
        H, W = gt.shape[:2]
        h, w = pred.shape[:2]
        pred = np.copy(pred)
        pred[:, :, 0] = pred[:, :, 0] / w * W
        pred[:, :, 1] = pred[:, :, 1] / h * H
        epe = np.sqrt(np.sum(np.square(numpy_resize(pred, H, W) - gt[:, :, :2]), axis=2))
        if gt.shape[-1] == 2:
            rows.append([np.mean(epe)])
            continue
        gmag = np.maximum(np.sqrt(np.sum(np.square(gt[:, :, :2]), axis=2)), 1e-10)
        rate = lambda m: np.logical_and(epe * m > 3, epe * m / gmag > 0.05).sum() / m.sum() * 100.   # noqa: E731
        valid, noc = gt[:, :, 2], gt[:, :, 3]
        row = [np.sum(epe * valid) / np.sum(valid), np.sum(epe * noc) / np.sum(noc),
               np.sum(epe * (valid - noc)) / max(np.sum(valid - noc), 1.0), rate(valid)]
        if moves is not None:
            mv, st = valid * moves[i], valid * (1.0 - moves[i])
            row += [np.sum(epe * mv) / np.sum(mv), np.sum(epe * st) / np.sum(st), rate(mv), rate(st)]
        rows.append(row)
    return np.asarray(rows, dtype=np.float64)


def bench_shape(shape, reps, warmup, rounds, dev):
    B, (h, w), (H, W), C, with_move = shape
    g = torch.Generator(device=dev).manual_seed(5)
    pred = 8.0 * torch.randn(B, 2, h, w, generator=g, device=dev)
    uv = 10.0 * torch.randn(B, 2, H, W, generator=g, device=dev)
    gt = uv
    if C == 4:
        valid = (torch.rand(B, 1, H, W, generator=g, device=dev) < 0.6).float()
        gt = torch.cat([uv, valid, valid * (torch.rand(B, 1, H, W, generator=g, device=dev) < 0.7).float()], dim=1)
    move = (torch.rand(B, H, W, generator=g, device=dev) < 0.4).float() if with_move else None
    gts = list(gt.cpu().numpy().transpose(0, 2, 3, 1))
    moves = None if move is None else list(move.cpu().numpy())

    sides = {"metrics_ms": lambda: ops.flow_metrics(gt, pred, move_mask=move),
             "metrics_flow_ms": lambda: ops.flow_metrics(gt, pred, move_mask=move, want_flow=True),
             "resize_ms": lambda: ops.flow_resize(pred, (H, W))}
    host = lambda: numpy_evaluate(gts, pred, moves)   # noqa: E731
    got = ops.flow_metrics(gt, pred, move_mask=move)[0].cpu().numpy()
    want = host()
    np.testing.assert_allclose(got[:, :want.shape[1]], want, rtol=1e-4)
    pooled = {k: [] for k in list(sides) + ["host_ms"]}
    with torch.no_grad():
        for _ in range(rounds):   # the sides alternate: clock and thermal drift lands on all of them alike
            for k, fn in sides.items():
                pooled[k] += timed(fn, reps, warmup)
            pooled["host_ms"] += timed_wall(host, max(reps // 4, 3), 1)
    out = {k: round(float(np.median(v)), 4) for k, v in pooled.items()}
    moved = 4.0 * B * (H * W * (C + (1 if with_move else 0)) + 2 * h * w)
    out["metrics_gbs"] = round(moved / out["metrics_ms"] / 1e6, 1)
    out["shape"] = [B, h, w, H, W, C, int(with_move)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sintel,kitti")
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
