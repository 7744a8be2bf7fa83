"""The item record of the distance-form sweep kernel (csrc/sweep_dist.hip: publish()): thread 0 of a workgroup decodes the next
queue item once and leaves (item, batch item, first pixel, flags) in LDS; every wave starts its pixel block from that record.

Each case runs algo="auto" through the NCHW entry on the smallest shape (C = 67) that reaches one path of the record and
compares with algo="direct" -- the gather kernel, which has no queue and no record -- at the bounds of tests/test_hip_parity.py
for that pair (log-DPV: 2e-4 abs + 2e-5 rel; depth: 1e-4 m at the 5 .. 40 m candidates of the synthetic batches).  A record
that names a wrong block, batch item or block shape puts whole blocks of 16 pixels at another place: errors of the size of
the values themselves.  Every call is made three times and the outputs must be the same bit for bit: a record left
from another item, or a queue counter left from another launch, shows as a difference between calls (ops.sweep_dpv takes a
workspace per call from the caching allocator: the third call runs on the first call's block, the second on a fresh one)."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from util import DEPTH_ATOL, to_dev

pytestmark = pytest.mark.gpu

LOGP_ATOL, LOGP_RTOL = 2e-4, 2e-5   # (tests/test_hip_parity.py: COST_ATOL, COST_RTOL)


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
    for what, a, r in zip(("cost", "logp", "depth"), runs[0], ref):
        assert (a is None) == (r is None), what
        if a is None:
            continue
        for again in runs[1:]:
            x = again[("cost", "logp", "depth").index(what)]
            assert np.array_equal(_bits(a), _bits(x)), (what, "differs between two calls", int((_bits(a) != _bits(x)).sum()))
        a, r = a.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(r)), what
        print(f"{what}: max |auto - direct| = {np.nanmax(np.abs(a - r)):.3e}")
        if what == "depth":
            np.testing.assert_allclose(a, r, rtol=0, atol=DEPTH_ATOL, equal_nan=True)
        else:
            np.testing.assert_allclose(a, r, rtol=LOGP_RTOL, atol=LOGP_ATOL, equal_nan=True)
    return off_fast_path


def test_workgroup_per_item_and_batch_item_change():
    """48 items: no queue, workgroup i decodes item i for itself at the start; the second half of them belong to batch item 1"""
    _check(_batch(801, 2, C=67, D=64, H=32, W=48, V=1, pose="mono"))


@pytest.mark.parametrize("pose", ["mono", "stereo"])   # (the probe picks 8x2 blocks for the first, 16x1 for the second)
def test_blocks_below_the_image_and_ragged_columns(pose):
    """H = 30: the last tile row has blocks below the image (skipped: the record's flag); W = 40: half of the last tile column
    lies beyond the image"""
    _check(_batch(802, 1, C=67, D=64, H=30, W=40, V=1, pose=pose))


def test_queue_with_stealing_and_a_routed_batch_item():
    """8 192 items (above the six per resident workgroup up to which a launch has no queue): pops, steals once a queue is dry,
    the change of batch item; batch item 1 is routed -- its blocks are skipped one by one, the gather kernel writes them"""
    off_fast_path = _check(_batch(803, 2, route=(1,), C=67, D=64, H=256, W=256, V=1, pose="mono"))
    assert off_fast_path > 0   # (the routed item's blocks are counted: it was routed)


def test_two_plane_groups_two_views():
    """D = 128: the instantiations with three workgroups per CU, two passes per view"""
    _check(_batch(804, 1, C=67, D=128, H=64, W=128, V=2, pose="mono"))


@pytest.mark.parametrize("want", [dict(want_cost=True, want_logp=False, want_depth=False), dict(want_logp=False, want_depth=True)])
def test_cost_only_and_depth_only_epilogues(want):
    """no log-DPV asked for: its stores go into an empty descriptor, and the wait that leaves them in flight must still cover
    the queue pop (cost only: the epilogue without the softmax)"""
    _check(_batch(801, 2, C=67, D=64, H=32, W=48, V=1, pose="mono"), **want)
