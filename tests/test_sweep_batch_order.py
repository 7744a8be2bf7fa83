"""The distance-form sweep kernel hands out the batch items of an NCHW call last to first (DIST_REV_BATCH,
csrc/sweep_dist_knobs.hpp; on in the product: the pack kernel wrote the last item last, profiles/r14_l2_warm/).  Which batch
item a pixel block belongs to changes nothing in its arithmetic, so every output must be the same bit for bit.

A library built with -DDIST_REV_BATCH=0 (the other objects from the product build) and the product library each run the
same seeded calls in a child process of their own; the parent compares costs, log-DPVs, depth maps and the kernel's count
of pixel blocks it left to the gather kernel or the direct evaluation.  The calls cover what the order has to get right:
the regular decode path (whole half-bands) on a forward motion and on a rectified pair, an image four tiles wide with
eight batch items, a shape off the regular path, two views at D = 128 (the D > 64 family), a routed item in the middle of
three -- its mark and its count hang on the batch item the queue thread decoded --, the depth-only and cost-only epilogues,
and a launch small enough to run a workgroup per pixel block.  Every other shape has more than DIST_ONE_EACH_X = 6 pixel
blocks per resident workgroup (B H W > 98 304), so that the queues run."""
import glob
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

CASES = ["mono_b2_256x512", "stereo_b2_256x512", "b8_256x64", "odd_b2_250x500", "v2_d128_b2_256x256", "b3_routed_middle",
         "b3_depth_only", "b3_cost_only", "one_each_b2_64x128"]

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

run("mono_b2_256x512", batch(41, 2, C=67, D=64, H=256, W=512, V=1, pose="mono"), want_cost=True)
run("stereo_b2_256x512", batch(42, 2, C=67, D=64, H=256, W=512, V=1, pose="stereo"), want_cost=True)
run("b8_256x64", batch(43, 8, C=67, D=64, H=256, W=64, V=1, pose="mono"), want_cost=True)
run("odd_b2_250x500", batch(44, 2, C=67, D=64, H=250, W=500, V=1, pose="mono"), want_cost=True)
run("v2_d128_b2_256x256", batch(45, 2, C=67, D=128, H=256, W=256, V=2, pose="mono"), want_cost=True)
d = batch(46, 3, route=(1,), C=67, D=64, H=256, W=512, V=1, pose="mono")
run("b3_routed_middle", d, want_cost=True)
run("b3_depth_only", d, want_logp=False)
run("b3_cost_only", d, want_cost=True, want_logp=False, want_depth=False)
run("one_each_b2_64x128", batch(47, 2, C=67, D=64, H=64, W=128, V=1, pose="mono"), want_cost=True)
torch.save(out, sys.argv[2])
"""


def _run_child(lib, path):
    env = dict(os.environ, PDEPTH_LIB=lib)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import torch
    return torch.load(path)


@pytest.fixture(scope="module")
def both_orders():
    """(first to last, the product) -> {case: (outputs, fallback_tiles)}: built and run once for all the cases"""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    others = sorted(o for o in glob.glob(os.path.join(CSRC, "*.o")) if os.path.basename(o) != "sweep_dist.o")
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "sweep_dist_fwd.o")
        lib = os.path.join(tmp, "libpdepth_fwd.so")
        r = subprocess.run([HIPCC, *FLAGS, "-DDIST_REV_BATCH=0", "-c", os.path.join(CSRC, "sweep_dist.hip"), "-o", obj],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj, *others],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        fwd = _run_child(lib, os.path.join(tmp, "fwd.pt"))
        rev = _run_child(os.path.join(REPO, "probabilistic-depth_amd", "libpdepth_hip.so"), os.path.join(tmp, "rev.pt"))
    assert sorted(fwd) == sorted(rev) == sorted(CASES)
    return fwd, rev


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_batch_order_outputs_bit_identical(both_orders, name):
    import torch
    fwd, rev = both_orders
    (f_out, f_fb), (r_out, r_fb) = fwd[name], rev[name]
    assert f_fb == r_fb, (name, "fallback_tiles", f_fb, r_fb)
    if name == "b3_routed_middle":
        assert r_fb > 0   # (the middle item was routed: its blocks are counted)
    some = False
    for what, a, b in zip(("cost", "logp", "depth"), f_out, r_out):
        assert (a is None) == (b is None), (name, what)
        if a is None:
            continue
        some = True
        assert a.shape == b.shape, (name, what)
        same = np.array_equal(a.numpy().view(np.int32), b.numpy().view(np.int32))
        assert same, (name, what, int((a.view(torch.int32) != b.view(torch.int32)).sum()))
    assert some, name
