"""Time of the DPV reductions on fp16 / bf16 logits (csrc/dpv_half.hip), against what a caller had to do before them: cast the
volume up with x.float() and run the fp32 reduction (forward), or run the fp32 backward and cast its result down (backward).

    python tools/bench_dpv_half.py [--shapes full,quarter] [--dtypes bf16,fp16] [--reps 50] [--warmup 5]

Prints ONE JSON line: per shape and dtype the median over --reps calls (device events, after --warmup calls; the two variants of
a pair alternate call by call, so that whatever else the machine does meets both) of
  fwd_cast_ms / fwd_ms : ops.dpv_reduce_ex(x.float(), want_logp, want_prob, want_depth)  /  the same on x, prob in fp32;
  fwd_lp_prob_ms       : the same on x with prob in x's dtype (prob_dtype=x.dtype), what the models ask for under autocast;
  bwd_cast_ms / bwd_ms : _native.dpv_reduce_backward(logp, g_logp, g_prob fp32, g_depth).to(dtype)  /
                         _native.dpv_reduce_backward_lp(..., g_prob in dtype);
  fwd_ratio, bwd_ratio : cast time over new time.  By algorithmic bytes per element at most 14/6 forward and 18/10 backward for
                         logp / g_logp alone; with prob and all three gradients, as timed here, 18/10 = 1.8 forward (18/8 = 2.25
                         with prob in the half type) and 22/12 = 1.83 backward.
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
from pdepth_amd import _native, ops, synth  # noqa: E402

SHAPES = {
    "full": dict(B=4, D=64, H=256, W=512),      # the decoder's last layer at the headline size
    "quarter": dict(B=4, D=64, H=64, W=128),    # _low_res_dpv at the same
}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def timed_pair(fns, reps, warmup):
    """Median ms of each callable, the callables alternating call by call."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [float(np.median(m)) for m in ms]


def bench(s, dtype, reps, warmup, dev):
    B, D, H, W = s["B"], s["D"], s["H"], s["W"]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, D, H, W, generator=g) * 8.0).to(dtype).to(dev)
    dc = torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0)).float().to(dev)
    kw = dict(want_logp=True, want_prob=True, want_depth=True)
    with torch.no_grad():
        fwd_cast, fwd, fwd_lp = timed_pair([lambda: ops.dpv_reduce_ex(x.float(), dc, **kw), lambda: ops.dpv_reduce_ex(x, dc, **kw),
                                            lambda: ops.dpv_reduce_ex(x, dc, prob_dtype=dtype, **kw)], reps, warmup)
        logp = ops.dpv_reduce_ex(x, dc)["logp"]
        g_logp = torch.randn(B, D, H, W, generator=g).to(dev)
        g_prob = torch.randn(B, D, H, W, generator=g).to(dev)
        g_prob_lp = g_prob.to(dtype)
        g_depth = torch.randn(B, H, W, generator=g).to(dev)
        bwd_cast, bwd = timed_pair(
            [lambda: _native.dpv_reduce_backward(logp, dc, g_logp=g_logp, g_prob=g_prob, g_depth=g_depth).to(dtype),
             lambda: _native.dpv_reduce_backward_lp(logp, dc, dtype, g_logp=g_logp, g_prob=g_prob_lp, g_depth=g_depth)], reps, warmup)
    r = lambda v: round(v, 4)
    return dict(fwd_cast_ms=r(fwd_cast), fwd_ms=r(fwd), fwd_lp_prob_ms=r(fwd_lp), fwd_ratio=round(fwd_cast / fwd, 3),
                fwd_lp_prob_ratio=round(fwd_cast / fwd_lp, 3), bwd_cast_ms=r(bwd_cast), bwd_ms=r(bwd), bwd_ratio=round(bwd_cast / bwd, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="full,quarter")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        out[name] = {"shape": SHAPES[name]}
        for dt in a.dtypes.split(","):
            out[name][dt] = bench(SHAPES[name], DTYPES[dt], a.reps, a.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
