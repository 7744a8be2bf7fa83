"""Which wave of a workgroup does what in the distance-form sweep kernel (csrc/sweep_dist.hip, sweep_dist_knobs.hpp).

The QUEUE THREAD -- lane 0 of wave DIST_QUEUE_WAVE, the wave with the short share of a pass's texel blocks -- resolves the pop
of the next item, decodes it into the record every wave starts the next block from, pops the item after it, counts the
blocks that leave the fast path and runs the leaving code; it does so in the item's FIRST PASS, behind its wave's last texel
block (DIST_DECODE_EARLY == 2), and on a path of its own where an item has no pass (a block below the image, a block of a
routed batch item).  The kq == 0 lanes of wave 0 store the block's depths; every wave ends the block with NC = 4 NH log-DPV
stores -- into an empty descriptor when no log-DPV is asked for -- and a wait that leaves them in flight.  A role that moved
wrongly shows as whole blocks of 16 pixels at another place, missing or stale (errors of the size of the values), as a queue
that hands an item out twice or not at all, or as a wrong count.

The pattern is tests/test_sweep_item_record.py's: algo="auto" through the NCHW entry against algo="direct" (the gather
kernel: no queue, no waves with roles) at the bounds of tests/test_hip_parity.py for that pair (log-DPV and cost: 2e-4 abs +
2e-5 rel; depth: 1e-4 m at the 5 .. 40 m candidates of the synthetic batches), and three calls whose outputs must be the
same bit for bit (a record, a queue counter or a store left from another block or launch differs between calls)."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from util import DEPTH_ATOL, to_dev

pytestmark = pytest.mark.gpu

LOGP_ATOL, LOGP_RTOL = 2e-4, 2e-5   # (tests/test_hip_parity.py: COST_ATOL, COST_RTOL)
NAMES = ("cost", "logp", "depth")


def _batch(seed, B, route=(), **kw):
    b = synth.make_batch(seed, B, **kw)
    if route:   # per-channel offsets of up to 6 sigma (bench.py: cfg2_routed): the statistics route these items to the gather kernel
        mu = (torch.rand(b["ref"].shape[1], generator=torch.Generator().manual_seed(5)) * 2 - 1) * 6.0
        for i in route:
            b["ref"][i] += mu[:, None, None]
            b["src"][i] += mu[None, :, None, None]
    return to_dev(b, "cuda")


def _bits(x):
    return x.cpu().numpy().view(np.int32)


def _check(d, **kw):
    """auto against direct, and auto three times over; -> the kernel's count of blocks that left the fast path"""
    B, _, H, W = d["ref"].shape
    args = (d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    runs = []
    for _ in range(3):
        runs.append(ops.sweep_dpv(*args, algo="auto", **kw))
        torch.cuda.synchronize()
    off_fast_path = _native.fallback_tiles(B, H, W)
    ref = ops.sweep_dpv(*args, algo="direct", **kw)
    for i, what in enumerate(NAMES):
        a, r = runs[0][i], ref[i]
        assert (a is None) == (r is None), what
        if a is None:
            continue
        for again in runs[1:]:
            assert np.array_equal(_bits(a), _bits(again[i])), (what, "differs between two calls", int((_bits(a) != _bits(again[i])).sum()))
        a, r = a.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(r)), what
        print(f"{what}: max |auto - direct| = {np.nanmax(np.abs(a - r)):.3e}")
        if what == "depth":
            np.testing.assert_allclose(a, r, rtol=0, atol=DEPTH_ATOL, equal_nan=True)
        else:
            np.testing.assert_allclose(a, r, rtol=LOGP_RTOL, atol=LOGP_ATOL, equal_nan=True)
    return off_fast_path


WANTS = {
    "depth_only": dict(want_cost=False, want_logp=False, want_depth=True),
    "logp_only": dict(want_cost=False, want_logp=True, want_depth=False),
    "cost_only": dict(want_cost=True, want_logp=False, want_depth=False),
    "all_three": dict(want_cost=True, want_logp=True, want_depth=True),
}


@pytest.mark.parametrize("pose", ["mono", "stereo"])   # (8x2 blocks for the first, 16x1 for the second)
@pytest.mark.parametrize("want", sorted(WANTS))
def test_outputs_asked_for(want, pose):
    """H = 30: blocks below the image (skipped: the next item is decoded on the skipped path); W = 40: a ragged last column,
    and with it blocks in which none of the lanes that store a depth is live (16x1: pixels 8 .. 15 of the last block of a
    row).  Depth only and cost only: the log-DPV stores go into an empty descriptor; log-DPV only: no depth store; cost only:
    the epilogue without the softmax, whose wait for the queue pop is another one.  Every combination must leave the same
    count of stores behind the pop that its wait assumes."""
    _check(_batch(811, 1, C=67, D=64, H=30, W=40, V=1, pose=pose), **WANTS[want])


@pytest.mark.parametrize("C", [3, 35, 67])   # NCHK = 0, 1, 2
def test_instantiations_one_plane_group(C):
    """the three D <= 64 instantiations (the decode stands inside their straight-line pass), on the ragged shape"""
    _check(_batch(812, 1, C=C, D=64, H=30, W=40, V=1, pose="mono"))


def test_planes_beyond_d():
    """D = 40: planes 40 .. 63 of the pass do not exist -- the waves that own them (2 and 3) store beyond the descriptor only,
    and their softmax partials are empty"""
    _check(_batch(813, 1, C=67, D=40, H=30, W=40, V=1, pose="mono"), want_cost=True)


def test_two_plane_groups_two_views():
    """D = 128, V = 2: NC = 8, and four passes per item, each with up to three attempts: the decode of the next item belongs
    to the first attempt of the first of them only"""
    _check(_batch(814, 1, C=67, D=128, H=16, W=32, V=2, pose="mono"))


def test_workgroup_per_item_and_batch_item_change():
    """B = 2, 32 x 48: 48 items, no queue -- workgroup i's queue thread decodes item i for itself at the start and never pops;
    the second half of the items belong to batch item 1"""
    _check(_batch(815, 2, C=67, D=64, H=32, W=48, V=1, pose="mono"))


def test_queue_stealing_and_the_routed_count():
    """B = 2, 256 x 256, batch item 1 routed: 8 192 items -- pops, steals once a queue is dry, the change of batch item, the
    routed item's blocks skipped one by one (the next item's record is still decoded and published on that path) and counted
    by the queue thread: every pixel block of the routed item, once -- four per 16 x 4 tile, the figure the kernel reported for
    this input before the roles could move"""
    B, H, W = 2, 256, 256
    off_fast_path = _check(_batch(803, B, route=(1,), C=67, D=64, H=H, W=W, V=1, pose="mono"))
    assert off_fast_path == 4 * ((W + 15) // 16) * ((H + 3) // 4) == 4096
