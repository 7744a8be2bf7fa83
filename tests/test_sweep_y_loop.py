"""The Y loop of the distance-form sweep kernel (csrc/sweep_dist.hip: `y_block`): a wave multiplies its q blocks of a pass out of
NS register sets; the blocks that have a successor NS blocks on run in a steady loop that always refills, the last ones
(fewer than 2 NS) behind it, each with the refills it still needs.  A refill into the wrong set, a block multiplied twice
or not at all, or a refill from beyond the wave's share puts whole rows of 16 texels of Y at the wrong values: errors of
the size of the costs themselves.

Each case runs algo="auto" through the NCHW entry (C = 67) against algo="direct" -- the gather kernel, which has no Y -- at
the bounds of tests/test_sweep_item_record.py (log-DPV: 2e-4 abs + 2e-5 rel; depth: DEPTH_ATOL; NaN patterns equal), and makes
every call three times: the outputs must be the same bit for bit.

Blocks of a wave in a pass (b1 - b0), counted once by a build with a counter in the kernel (not kept); "count: waves x passes",
and the passes that did not fit their blocks (`go` false: at D <= 64 evaluated directly in the kernel, at D > 64 tried again
in halves).  A wave with n blocks runs max(0, n - 2 NS + 1) blocks in the steady loop and the rest behind it:

    case                    NS   0: ..  1: ..  2: ..  3: ..  4: ..  5: ..  6: ..  7: ..  8: ..  9: ..    did not fit
    stereo-32x48             1     45    204    135                                                            0
    mono-32x48               1     54    266     64                                                            0
    wide-64x128              1    106    198    398    825    408    104      9                                0
    wide-128x256             1     87    297    522   1015   1803   1462   1058                             1948 (844 direct)
    wide-D128-V2-64x128      2    860   3932   1188   1506    555     87                                      64
    wide-D128-128x256        2   1399   2825   4950   1349   1461   1542   1293    901    465    111         232

The forward motion of pose="mono" on these image sizes stays at 0 .. 2 blocks per wave (H = 64, W = 128: 342 / 718 / 988; D = 128,
V = 2: 1397 / 5319 / 1476; it takes 256x512 to reach 6), hence pose="wide" for the longer trip counts: NS = 1 with 1 .. 5 steady
iterations, NS = 2 with 1, 2, 3 blocks (no steady iteration), 4 and 5 (one, then 2 or 3 blocks: the third is the refill issued
behind the loop), 6 .. 9 (two and three).
"""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from util import DEPTH_ATOL, to_dev

pytestmark = pytest.mark.gpu

LOGP_ATOL, LOGP_RTOL = 2e-4, 2e-5   # (tests/test_sweep_item_record.py)

def _case(seed, pose, D, H, W, V=1):
    return dict(seed=seed, B=1, C=67, D=D, H=H, W=W, V=V, pose=pose)


CASES = {
    "stereo-32x48": _case(811, "stereo", 64, 32, 48),
    "mono-32x48": _case(812, "mono", 64, 32, 48),
    "wide-64x128": _case(815, "wide", 64, 64, 128),
    "wide-128x256": _case(815, "wide", 64, 128, 256),   # (with passes that do not fit: the in-kernel direct evaluation)
    "wide-D128-V2-64x128": _case(817, "wide", 128, 64, 128, V=2),
    "wide-D128-128x256": _case(817, "wide", 128, 128, 256),
}


def _bits(x):
    return x.cpu().numpy().view(np.int32)


def _check(case):
    kw = dict(case)
    d = to_dev(synth.make_batch(kw.pop("seed"), kw.pop("B"), **kw), "cuda")
    args = (d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    runs = []
    for _ in range(3):
        runs.append(ops.sweep_dpv(*args, algo="auto"))
        torch.cuda.synchronize()
    B, _, H, W = d["ref"].shape
    print("passes evaluated directly in the kernel:", _native.fallback_tiles(B, H, W))
    ref = ops.sweep_dpv(*args, algo="direct")
    seen = 0
    for i, what in enumerate(("cost", "logp", "depth")):
        a, r = runs[0][i], ref[i]
        assert (a is None) == (r is None), what
        if a is None:
            continue
        seen += 1
        for again in runs[1:]:
            assert np.array_equal(_bits(a), _bits(again[i])), (what, "differs between two calls", int((_bits(a) != _bits(again[i])).sum()))
        a, r = a.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(r)), what
        print(f"{what}: max |auto - direct| = {np.nanmax(np.abs(a - r)):.3e}")
        if what == "depth":
            np.testing.assert_allclose(a, r, rtol=0, atol=DEPTH_ATOL, equal_nan=True)
        else:
            np.testing.assert_allclose(a, r, rtol=LOGP_RTOL, atol=LOGP_ATOL, equal_nan=True)
    assert seen >= 2   # (log-DPV and depth)


@pytest.mark.parametrize("case", sorted(CASES))
def test_auto_against_direct_three_times_over(case):
    _check(CASES[case])
