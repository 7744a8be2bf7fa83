"""GPU: the sweep's reductions over the four K-slice lanes of a pixel (csrc/wave_util.hpp: quad_sum, quad_max; csrc/sweep_dist.hip:
the centring and the partial softmax) and the fold of its row table over groups of eight lanes (DIST_ROWTAB_FOLD).

1. tools/mb_lane_exchange.hip, built and run here: v_permlane16_swap / v_permlane32_swap against ds_swizzle + ds_bpermute, bit
   for bit, on random values and on +0, -0, +inf, -inf and NaN in every lane position, alone and beside
   v_mfma_f32_16x16x32_f16 and LDS atomics in the other waves of the SIMD: zero mismatches in both settings.  (The kernel
   uses the LDS pipe -- profiles/r15_lane_exchange/ --; the swaps stay buildable behind DIST_LANE_XCHG=1.)
2. The distance-form kernel (algo="dist") against the CPU oracle, with the comparison and the tolerances of
   tests/test_hip_parity.py::test_sweep_matches_oracle, on shapes of a few pixel blocks: 8 x 32 and 6 x 20 (an edge block with
   dead lanes), C = 8, 35, 67 (no / one / two whole chunks of 32 channels: the three instantiations of the centring), D = 16
   (three waves' partial maxima -inf, their sums 0), 64, and 96 (two passes; the planes beyond D masked in the second), mono
   (16 x 1 blocks) and stereo (8 x 2: the fold's groups of eight lanes are the block's two pixel rows; at 6 x 20 some of their
   lanes are dead).  One case carries a NaN feature in one pixel: NaN comes out where the oracle has it."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops, synth
from util import DEPTH_ATOL, oracle_batch, to_dev

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
COST_ATOL, COST_RTOL = 2e-4, 2e-5   # (tests/test_hip_parity.py)


def test_swaps_and_lds_exchanges_are_the_same_bits(tmp_path):
    exe = str(tmp_path / "mb_lane_exchange")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I",
                        os.path.join(REPO, "probabilistic-depth_amd", "csrc"), "-o", exe, os.path.join(REPO, "tools", "mb_lane_exchange.hip")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    found = dict(re.findall(r"^(alone|loaded)\s*: mismatches (\d+)", r.stdout, re.M))
    assert found == {"alone": "0", "loaded": "0"}, r.stdout


_ORACLE = {}


def _case(H, W, C, D, pose, nan_at=None):
    key = (H, W, C, D, pose, nan_at)
    if key not in _ORACLE:
        b = synth.make_batch(1500 + C + D, 1, C=C, D=D, H=H, W=W, V=1, pose=pose)
        if nan_at is not None:
            c, y, x = nan_at
            b["ref"][0, c, y, x] = float("nan")
        _ORACLE[key] = (b, oracle_batch(b, "L2"))
    return _ORACLE[key]


def _compare(b, oracle):
    ocost, ologp, odepth = oracle
    d = to_dev(b, "cuda")
    args = (d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    cost, logp, depth = ops.sweep_dpv(*args, feat_dist="L2", want_cost=True, algo="dist")
    # (assert_allclose: a NaN on one side only is a mismatch)
    np.testing.assert_allclose(cost.cpu().numpy(), ocost.numpy(), rtol=COST_RTOL, atol=COST_ATOL)
    np.testing.assert_allclose(logp.cpu().numpy(), ologp.numpy(), rtol=COST_RTOL, atol=COST_ATOL)
    dn, on = depth.cpu().numpy(), odepth.numpy()
    assert np.array_equal(np.isnan(dn), np.isnan(on))
    err = float(np.nanmax(np.abs(dn - on)))
    print(f"max |cost - oracle| {np.nanmax(np.abs(cost.cpu().numpy() - ocost.numpy())):.2e}, max |depth - oracle| {err:.2e}")
    assert err <= DEPTH_ATOL, f"depth differs from the CPU oracle by {err:.3e}"
    # depth-only request: the epilogue without the log-DPV
    _, _, depth3 = ops.sweep_dpv(*args, feat_dist="L2", want_cost=False, want_logp=False, want_depth=True, algo="dist")
    assert np.array_equal(depth3.cpu().numpy().view(np.int32), dn.view(np.int32))
    return cost, logp, depth


@pytest.mark.parametrize("pose", ["mono", "stereo"])
@pytest.mark.parametrize("D", [16, 64, 96])
@pytest.mark.parametrize("C", [8, 35, 67])
@pytest.mark.parametrize("H,W", [(8, 32), (6, 20)])
def test_dist_sweep_matches_oracle_on_small_blocks(H, W, C, D, pose):
    b, oracle = _case(H, W, C, D, pose)
    assert bool(torch.isfinite(oracle[0]).all())
    _compare(b, oracle)


def test_nan_feature_comes_out_where_the_oracle_has_it():
    H, W, C, D = 6, 20, 67, 64
    y, x = 3, 17   # (in the edge block of its row: lanes beside it are dead)
    b, oracle = _case(H, W, C, D, "mono", nan_at=(5, y, x))
    ocost, ologp, odepth = oracle
    want = np.zeros((H, W), dtype=bool)
    want[y, x] = True
    # the oracle: that pixel, every plane, and nothing else
    assert np.array_equal(np.isnan(ocost.numpy()), np.broadcast_to(want, (1, D, H, W)))
    assert np.array_equal(np.isnan(ologp.numpy()), np.broadcast_to(want, (1, D, H, W)))
    assert np.array_equal(np.isnan(odepth.numpy()), want[None])
    cost, logp, depth = _compare(b, oracle)
    assert np.array_equal(np.isnan(cost.cpu().numpy()), np.isnan(ocost.numpy()))
    assert np.array_equal(np.isnan(logp.cpu().numpy()), np.isnan(ologp.numpy()))
