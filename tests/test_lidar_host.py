"""CPU suite of the LiDAR ground-truth path (csrc/lidar_depth.hip, ops.lidar_depth, utils/lidar.py, harness.targets_from_lidar):
the case generator of tests/util_lidar.py produces inputs on which no fp32 rounding can flip a decision, the C entries refuse bad
arguments before any launch, generate_depth refuses the beam resampling, and the compiler's output has no spill and no scratch.

There is no golden fixture from the reference's generate_depth: its extension needs Eigen, OpenCV and pybind11's Eigen bridge,
which are not available where these tests run.  The contract is the source (external/utils_lib/python/utils_lib.cpp:86-160,
kittiloader/kitti.py:683-729), restated in float64 and in two fp32 summation orders in tests/util_lidar.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, harness, ops
from pdepth_amd.utils import lidar

import util_lidar as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")
KEYS = ("dmap", "mask", "dmap_quarter", "mask_quarter")
# (seed, points, H, W, filtering, half field of view in degrees): the training shape with a full turn of the sensor, the GPU suite's
# contended scan, an odd image
CASES = [(11, 128000, 256, 768, 2, 180.0), (12, 20000, 64, 192, 2, 50.0), (13, 20000, 64, 192, 4, 50.0), (14, 6000, 37, 53, 0, 40.0)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "seed%d_%dx%d_f%d" % (c[0], c[2], c[3], c[4]))
def case(request):
    seed, n, H, W, f, fov = request.param
    M, intr = U.calibration(H, W)
    raw = U.synthetic_scan(seed, n, fov)
    pts, stats = U.prune(raw, M, intr, H, W, f)
    _, M32, I32 = U.cast_inputs(pts, M, intr)
    return {"raw": raw, "pts": pts, "M": M32, "intr": I32, "H": H, "W": W, "f": f, "stats": stats}


def test_fp32_position_error_is_inside_the_bound(case):
    """Both fp32 orders (separate products and sums; fused multiply-adds) against float64, on every point of the unpruned scan
    that could be kept (cam_z > 0.05: behind the camera the position means nothing)."""
    pts, M, intr = U.cast_inputs(case["raw"], case["M"], case["intr"])
    cam, _, uf, vf = U.project64(pts, M, intr)
    du, dv, dz = U.position_bound(pts, M, intr)
    live = cam[:, 2] > 0.05
    assert live.sum() > 100
    for fused in (False, True):
        z32, u32, v32 = U.project32(pts, M, intr, fused)
        eu, ev, ez = np.abs(u32 - uf)[live], np.abs(v32 - vf)[live], np.abs(z32 - cam[:, 2])[live]
        idx, _ = U.pixels(cam[:, 2], uf, vf, case["H"], case["W"])
        print("fused" if fused else "separate", "max position error of in-image points [px]:",
              max(np.abs(u32 - uf)[idx].max(), np.abs(v32 - vf)[idx].max()), "max |dz| [m]:", ez.max())
        assert (eu <= du[live]).all() and (ev <= dv[live]).all() and (ez <= dz[live]).all()


def test_pruned_case_has_one_answer(case):
    """On the pruned points both fp32 restatements give exactly the float64 non-zero pattern of all four outputs, and depths
    inside the chain's rounding."""
    H, W, f = case["H"], case["W"], case["f"]
    want = U.reference(case["pts"], case["M"], case["intr"], H, W, f)
    removed_by_filter = int((want["zbuf"] != 0).sum() - (want["dmap"] != 0).sum())
    print("occupied pixels:", int((want["zbuf"] != 0).sum()), "cleared by the filter and the border:", removed_by_filter)
    assert removed_by_filter > 0 and (want["dmap"] != 0).sum() > 100   # a wrong filter is visible
    for fused in (False, True):
        got = U.reference(case["pts"], case["M"], case["intr"], H, W, f, dtype=U.F32, fused=fused)
        for k in KEYS:
            assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
            assert np.array_equal(got[k] != 0, want[k] != 0), (k, fused)
        assert (np.abs(got["dmap"] - want["dmap"]) <= want["tol"]).all()


def test_generator_removes_at_most_two_percent(case):
    """A condition on the inputs, not a tolerance: the pruning must leave the scan a scan."""
    s = case["stats"]
    print(s)
    assert s["in_image"] > 500
    assert s["removed_in_image"] <= 0.02 * s["in_image"], s


def test_argument_validation_without_gpu():
    lib = _native.load()
    ws_bytes = lib.pdepth_lidar_depth_workspace_bytes
    assert ws_bytes(2, 37, 53) == (2 * 37 * 53 * 4 + 255) // 256 * 256
    assert ws_bytes(0, 37, 53) == 0 and ws_bytes(1, -1, 53) == 0 and ws_bytes(1, 37, 0) == 0
    need = ws_bytes(1, 8, 8)
    f = ctypes.c_float

    def call(points=16, counts=16, M=16, intr=16, B=1, Nmax=4, dim=4, Mb=0, Ib=0, H=8, W=8, filt=2, fd=1.0, pd=1000.0, dmap=16, mask=16,
             dq=16, mq=16, ws=256, nbytes=need):
        rc = lib.pdepth_lidar_depth_f32(points, counts, M, intr, B, Nmax, dim, Mb, Ib, H, W, filt, f(fd), f(pd), dmap, mask, dq, mq, ws,
                                        nbytes, None)
        return rc, lib.pdepth_last_error()

    for kw in ({"points": None}, {"counts": None}, {"M": None}, {"intr": None}):
        rc, msg = call(**kw)
        assert rc == 1 and b"null pointer" in msg, (kw, msg)
    for kw in ({"dmap": None}, {"mask": None}, {"dq": None}, {"mq": None}):
        rc, msg = call(**kw)
        assert rc == 1 and b"null output" in msg, (kw, msg)
    for kw in ({"B": 0}, {"H": 0}, {"W": -3}):
        rc, msg = call(**kw)
        assert rc == 1 and b"non-positive" in msg, (kw, msg)
    rc, msg = call(Nmax=-1)
    assert rc == 1 and b"negative Nmax" in msg
    rc, msg = call(dim=5)
    assert rc == 1 and b"point_dim" in msg
    rc, msg = call(points=20)
    assert rc == 1 and b"16-byte aligned" in msg
    for filt in (-1, 5):
        rc, msg = call(filt=filt)
        assert rc == 1 and b"filtering must be in 0 .. 4" in msg
    for kw in ({"fd": float("nan")}, {"fd": float("inf")}, {"pd": float("nan")}):
        rc, msg = call(**kw)
        assert rc == 1 and b"finite" in msg, (kw, msg)
    rc, msg = call(nbytes=need - 1)
    assert rc == 3 and b"workspace" in msg
    assert call(ws=None)[0] == 3
    rc, msg = call(ws=264)
    assert rc == 3 and b"aligned" in msg
    # an image without a quarter map needs no quarter outputs: the next refusal (the workspace) is reached
    assert call(H=3, W=8, dq=None, mq=None, ws=None)[0] == 3


def test_python_layers_refuse_before_any_launch():
    pts, counts = torch.zeros(1, 5, 4), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lidar_depth(pts, counts, torch.eye(4), torch.zeros(3, 3), 8, 8)
    with pytest.raises(RuntimeError, match=r"points must be \[B,Nmax,4\]"):
        ops.lidar_depth(torch.zeros(5, 4), counts, torch.eye(4), torch.zeros(3, 4), 8, 8)
    with pytest.raises(RuntimeError, match="counts"):
        ops.lidar_depth(pts, torch.zeros(2, dtype=torch.int32), torch.eye(4), torch.zeros(3, 4), 8, 8)
    with pytest.raises(RuntimeError, match="M_velo2cam"):
        ops.lidar_depth(pts, counts, torch.eye(3), torch.zeros(3, 4), 8, 8)
    with pytest.raises(NotImplementedError, match="pool"):
        ops.lidar_depth(pts, counts, torch.eye(4), torch.zeros(3, 4), 8, 8, pool=2)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.lidar_depth(pts.clone().requires_grad_(), counts, torch.eye(4), torch.zeros(3, 4), 8, 8)


def test_generate_depth_refuses_the_beam_resampling():
    class Attr:
        filtering, upsample = 2, 4

    pts = np.zeros((5, 4))
    for params in ({"filtering": 2, "upsample": 1}, {"filtering": 2, "upsample": 0.5, "filterdiff": 1}, Attr()):
        with pytest.raises(NotImplementedError, match="upsample"):
            lidar.generate_depth(pts, np.zeros((3, 4)), np.eye(4), 8, 8, params)
        with pytest.raises(NotImplementedError, match="upsample_velodyne"):
            harness.targets_from_lidar(torch.zeros(1, 5, 4), torch.zeros(1, dtype=torch.int32), torch.eye(4), torch.zeros(3, 4), 8, 8, params)


def _metadata(name):
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc here")
    r = subprocess.run(["make", "-C", CSRC, name + ".s"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(CSRC, name + ".s")).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        block = m.group(0)
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_lidar_kernels_no_spills_no_scratch():
    """Read from the code-object metadata of `make lidar_depth.s` and `make clear.s` alone: the point kernel and the map kernel in
    its five instantiations (filtering 0 .. 4), and the fill kernel that clears the z-buffer (csrc/clear.hip, shared with every
    scatter of the library)."""
    ks = _metadata("lidar_depth")
    assert len([n for n in ks if "lidar_points_kernel" in n]) == 1 and len([n for n in ks if "lidar_maps_kernel" in n]) == 5, sorted(ks)
    assert len(ks) == 6, sorted(ks)
    fill = _metadata("clear")
    assert len(fill) == 1 and "fill32_kernel" in next(iter(fill)), sorted(fill)
    ks.update(fill)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256, (name, md)
        # a 32 x 32 tile with a halo of up to 4 pixels: under 8 KiB of LDS, four workgroups per CU keep their registers (512 / 4)
        assert md["group_segment_fixed_size"] <= 8192 and md["vgpr_count"] <= 128, (name, md)
