"""The distance-form sweep kernel with and without the prefetch of the next pixel block's inputs (DIST_PREFETCH,
csrc/sweep_dist_knobs.hpp; off in the product): the arithmetic is the same, so every output must be the same bit for bit.

A library built with -DDIST_PREFETCH=1 (the other objects from the product build) and the product library each run the
same seeded calls in a child process of their own; the parent compares costs, log-DPVs, depth maps and the kernel's count
of passes it left to the direct evaluation.  The calls cover what the prefetch has to get right: consecutive blocks of
different batch items and a routed (skipped) item between them, blocks below the image and clamped pixels (H, W not
multiples of 4 / 16), two views at D = 128 (the D > 64 family), the depth-only and cost-only epilogues, and a launch
small enough to run a workgroup per pixel block (nothing is prefetched there)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm",
         "-amdgpu-atomic-optimizer-strategy=None", "-Wno-unused-function", "-Wno-inline-asm"]
OBJS = ["capi.o", "sweep_direct.o", "sweep_pack.o", "pack_dist.o", "sweep_tiled.o", "dpv.o", "warp.o", "dpv_fuse.o",
        "dpv_moments.o", "correlation.o", "inverse_warp.o", "correlation_general.o", "ufield.o", "sweep_bwd.o", "dpv_bwd.o", "clear.o", "sweep_tiled_n2.o"]

CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import pdepth_amd
from pdepth_amd import ops, synth, _native

def batch(seed, B, route=(), **kw):
    b = synth.make_batch(seed, B, **kw)
    if route:   # per-channel offsets of up to 6 sigma (bench.py: cfg2_routed): the guard routes these items to the gather kernel
        mu = (torch.rand(b["ref"].shape[1], generator=torch.Generator().manual_seed(5)) * 2 - 1) * 6.0
        for i in route:
            b["ref"][i] += mu[:, None, None]
            b["src"][i] += mu[None, :, None, None]
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}

out = {}
def run(name, d, **kw):
    dc = ops.d_candi_tensor(d["d_candi"], "cuda")
    r = ops.sweep_dpv(d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc, 10.0, **kw)
    torch.cuda.synchronize()
    B, _, H, W = d["ref"].shape
    out[name] = ([None if x is None else x.cpu() for x in r], _native.fallback_tiles(B, H, W))

d = batch(31, 3, route=(1,), C=67, D=64, H=256, W=512, V=1, pose="mono")
run("b3_routed_middle", d, want_cost=True)
run("b3_depth_only", d, want_logp=False)
run("b3_cost_only", d, want_cost=True, want_logp=False, want_depth=False)
run("odd_250x500", batch(32, 2, C=67, D=64, H=250, W=500, V=1, pose="mono"), want_cost=True)
run("odd_stereo_250x500", batch(33, 2, C=67, D=64, H=250, W=500, V=1, pose="stereo"), want_cost=True)
run("v2_d128", batch(34, 2, C=67, D=128, H=256, W=256, V=2, pose="mono"), want_cost=True)
run("c22_d83", batch(35, 2, C=22, D=83, H=254, W=250, V=3, pose="wide"), want_cost=True)
run("one_each_64x128", batch(36, 1, C=67, D=64, H=64, W=128, V=1, pose="mono"), want_cost=True)
torch.save(out, sys.argv[2])
"""


def _run_child(lib, path):
    env = dict(os.environ, PDEPTH_LIB=lib)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import torch
    return torch.load(path)


@pytest.mark.gpu
def test_prefetch_outputs_bit_identical():
    import torch
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "sweep_dist_pf.o")
        lib = os.path.join(tmp, "libpdepth_pf.so")
        r = subprocess.run([HIPCC, *FLAGS, "-DDIST_PREFETCH=1", "-c", os.path.join(CSRC, "sweep_dist.hip"), "-o", obj],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj, *[os.path.join(CSRC, o) for o in OBJS]],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        old = _run_child(os.path.join(REPO, "probabilistic-depth_amd", "libpdepth_hip.so"), os.path.join(tmp, "old.pt"))
        new = _run_child(lib, os.path.join(tmp, "new.pt"))
    assert old.keys() == new.keys()
    assert old["b3_routed_middle"][1] > 0   # (the middle item was routed: its blocks are counted)
    for name in old:
        (o_out, o_fb), (n_out, n_fb) = old[name], new[name]
        assert o_fb == n_fb, (name, "fallback_tiles", o_fb, n_fb)
        for what, a, b in zip(("cost", "logp", "depth"), o_out, n_out):
            assert (a is None) == (b is None), (name, what)
            if a is None:
                continue
            assert a.shape == b.shape, (name, what)
            same = np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))
            assert same, (name, what, int((a.view(torch.int32) != b.view(torch.int32)).sum()))
