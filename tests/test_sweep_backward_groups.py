"""The g_src pass of csrc/sweep_bwd.hip where a (tile, view) pair does not fit one LDS box image: groups of planes that split
(re-zeroed image, a new box origin), planes added directly to global memory (their own channel tail), runs of planes with no
in-bounds tap.  The poses of synth.make_pose move the source camera away from the planes, the warp only shrinks and every pair
of tests/test_sweep_backward.py is one group (asserted below); the cases here (util_sweep_backward.group_cases) put the source
camera in front of the reference one.  A host restatement of the grouping (util_sweep_backward.tile_groups) says which paths
each case takes -- checked without a GPU -- and tells the GPU tests where to look."""
import pytest
import torch

from pdepth_amd import synth
import util_sweep_backward as U
from util_sweep_backward import hip_grads, l1_allowance, oracle_grads, rel_err, to_dev

SIGMA = 10.0
TOL = 1e-4          # rel_err of a gradient against float64 (tests/test_sweep_backward.py)
TOL_ORDER = 1e-6    # g_src between two calls: the order of the atomic adds (test_gradients_reproducible)
NAMES = ("A", "C", "E", "R")
METRICS = ("L2", "L1")

_memo = {}


def _cases():
    if "cases" not in _memo:
        _memo["cases"] = U.group_cases()
        assert tuple(_memo["cases"]) == NAMES
    return _memo["cases"]


def _groups(name):
    if ("groups", name) not in _memo:
        cap, tile = U.kernel_constants()
        _memo[("groups", name)] = U.tile_groups(_cases()[name], cap, tile)
    return _memo[("groups", name)]


def _interesting(tg):
    """The pairs that leave the one-group path: a direct plane or at least two groups."""
    return {key: gs for key, gs in tg.items() if len(gs) >= 2 or any(g[0] == "direct" for g in gs)}


# ---- without a GPU: the restatement, and what the cases reach ----------------------------------------------------------
def test_kernel_constants_are_found():
    cap, tile = U.kernel_constants()
    assert cap > 0 and tile > 0
    assert cap >= (tile + 1) ** 2   # an unmagnified tile (its taps: tile + 1 texels a side) fits: the ordinary poses stage


def test_group_planes_on_hand_made_boxes():
    none = (U._BIG, -U._BIG, U._BIG, -U._BIG)
    sq = lambda x, y, n: (x, x + n - 1, y, y + n - 1)   # noqa: E731
    # 10 x 10 boxes under a cap of 150: two that overlap share a group (12 x 12), a third far away starts another
    assert U.group_planes([sq(0, 0, 10), sq(2, 2, 10), sq(50, 0, 10)], 150) == [
        ("staged", 0, 2, (0, 11, 0, 11)), ("staged", 2, 3, (50, 59, 0, 9))]
    # area == cap still fits; one texel more does not
    assert U.group_planes([(0, 14, 0, 9)], 150) == [("staged", 0, 1, (0, 14, 0, 9))]
    assert U.group_planes([(0, 14, 0, 10)], 164) == [("direct", 0, (0, 14, 0, 10))]
    # planes without a tap join the group they stand in and never split it; alone they are an empty run; an empty run in front
    # of an oversized plane ends there, the oversized plane goes alone, what follows starts a new group
    assert U.group_planes([none, sq(0, 0, 10), none, sq(1, 1, 10), none], 150) == [("staged", 0, 5, (0, 10, 0, 10))]
    assert U.group_planes([none, none], 150) == [("empty", 0, 2)]
    assert U.group_planes([none, none, sq(0, 0, 13), sq(0, 0, 5), none], 150) == [
        ("empty", 0, 2), ("direct", 2, (0, 12, 0, 12)), ("staged", 3, 5, (0, 4, 0, 4))]


def test_plane_boxes_clip_to_the_image_and_to_the_live_pixels():
    import numpy as np
    H, W, tile = 5, 6, 4   # tiles: 2 x 2, the last ones 1 row / 2 columns live
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ix, iy = 2 * xs - 3.5, ys + 0.25                      # plane 0: x doubles and moves left, y a quarter texel down
    nan = np.full_like(ix, np.nan)
    x_lo, x_hi, y_lo, y_hi = U.plane_boxes(np.stack([ix, nan]), np.stack([iy, iy]), H, W, tile)
    # tile (0, 0): pixels x 0..3 -> ix -3.5, -1.5, 0.5, 2.5: taps -4..3, in bounds 0..3; y 0..3 -> taps 0..4
    assert (x_lo[0, 0, 0], x_hi[0, 0, 0], y_lo[0, 0, 0], y_hi[0, 0, 0]) == (0, 3, 0, 4)
    # tile (1, 1): pixels x 4..5 -> ix 4.5, 6.5: taps 4, 5 (6 and 7 are out); y 4 -> taps 4 (5 is out)
    assert (x_lo[0, 1, 1], x_hi[0, 1, 1], y_lo[0, 1, 1], y_hi[0, 1, 1]) == (4, 5, 4, 4)
    assert (x_lo[1] > x_hi[1]).all() and (y_lo[1] > y_hi[1]).all()   # a position that is not finite has no tap


def test_cases_reach_the_split_direct_and_empty_paths():
    """Conditions on the INPUTS of the GPU tests below (not measurements of the kernel): what the restatement finds over the
    case set.  A, of 60 pairs: 41 staged groups, 2 direct planes (C = 11: channel tail), one pair of 3 groups, one that splits
    in two staged groups, 20 empty pairs.  C: one pair that splits in two staged groups, no direct plane.  E: an empty run
    followed by a direct plane.  R: 39 direct planes, 10 pairs of 3 or more groups, 13 pairs that split without a direct plane."""
    cap, tile = U.kernel_constants()
    total = {}
    for name in NAMES:
        b = _cases()[name]
        assert float(b["d_candi"].min() + b["t"][..., 2].min()) >= 1.0, name   # no plane near the camera plane
        st = U.group_stats(_groups(name), b["src"].shape[2])
        print(name, tuple(b["src"].shape), st)
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    assert total["direct"] >= 2 and total["direct_with_channel_tail"] >= 1, total
    assert total["pairs_3_groups"] >= 2, total
    assert total["pairs_split_no_direct"] >= 1, total
    assert total["pairs_all_empty"] >= 1, total
    assert total["empty_then_group"] >= 1, total
    # each case is here for a reason of its own
    sa, sc, se, sr = (U.group_stats(_groups(n), _cases()[n]["src"].shape[2]) for n in NAMES)
    assert sa["direct"] >= 2 and sa["direct_with_channel_tail"] >= 2 and sa["pairs_all_empty"] >= 1, sa
    assert sc["direct"] == 0 and sc["pairs_split_no_direct"] >= 1, sc
    assert se["empty_then_group"] >= 1, se
    assert sr["pairs_3_groups"] > sa["pairs_3_groups"] and sr["pairs_split_no_direct"] > sa["pairs_split_no_direct"], sr
    items = {key[0] for key in _interesting(_groups("R"))}
    assert items == {0, 1}, items   # both batch items of R leave the one-group path


def test_the_ordinary_poses_form_one_group_per_pair():
    """Why the cases above exist: every (tile, view) pair of the inputs of tests/test_sweep_backward.py is a single group and
    has no direct plane -- at 24 x 40 no box can exceed the cap, and away-moving poses only shrink the warp."""
    from test_sweep_backward import CASES
    cap, tile = U.kernel_constants()
    assert 24 * 40 <= cap
    seen = set()
    inputs = []
    for metric, V, C, D, pose, cx_off in CASES:
        if (V, D, pose, cx_off) not in seen:   # (the grouping does not depend on the features: C = 1)
            seen.add((V, D, pose, cx_off))
            inputs.append(synth.make_batch(23, 2, C=1, D=D, H=24, W=40, V=V, pose=pose, cx_off=cx_off))
    inputs.append(synth.make_batch(26, 2, C=1, D=64, H=64, W=96, V=2, pose="stereo"))   # test_gradients_reproducible
    inputs.append(synth.make_batch(3100, 2, C=1, D=64, H=64, W=96, V=1, pose="mono"))    # a sweep of the model test's size
    for b in inputs:
        for key, gs in U.tile_groups(b, cap, tile).items():
            assert len(gs) == 1 and gs[0][0] in ("staged", "empty"), (key, U.describe(gs))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _gup(b, dev):
    B, V, C, H, W = b["src"].shape
    return torch.randn(B, len(b["d_candi"]), H, W, generator=torch.Generator().manual_seed(5)).to(dev)


def _result(dev, name, metric):
    """Everything the tests of one (case, metric) share, computed once: the float64 and fp32 oracle gradients, the L1
    allowance, the HIP gradients of the both-outputs call.  Nothing in it is written to afterwards."""
    key = ("result", name, metric)
    if key not in _memo:
        b = _cases()[name]
        gup = _gup(b, dev)
        r64, s64 = oracle_grads(b, gup, SIGMA, metric, torch.float64, dev)
        r32, s32 = oracle_grads(b, gup, SIGMA, metric, torch.float32, dev)
        ar, as_ = l1_allowance(b, gup, SIGMA, dev) if metric == "L1" else (None, None)
        d = to_dev(b, dev)
        gr, gs, _ = hip_grads(d, gup, SIGMA, metric)
        _memo[key] = dict(b=b, d=d, gup=gup, r64=r64, s64=s64, r32=r32, s32=s32, ar=ar, as_=as_, gr=gr, gs=gs)
    return _memo[key]


def _src_errs(g, r):
    """rel_err of a g_src over the whole tensor, then of each view against that view's own max |g64|."""
    out = [rel_err(g, r["s64"], r["as_"])]
    for v in range(g.shape[1]):
        out.append(rel_err(g[:, v], r["s64"][:, v], None if r["as_"] is None else r["as_"][:, v]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_float64_oracle(dev, name, metric):
    """g_ref, g_src and each view of g_src (against that view's own max |g64|, so that an error in the magnified view cannot
    hide behind the other) within 1e-4 of float64.  Autograd of the oracle in fp32 is at 1e-6 (g_ref) and 5e-6 ... 9e-6 (g_src)
    on these cases; the figures of both are printed on every run."""
    r = _result(dev, name, metric)
    e32 = [rel_err(r["r32"], r["r64"], r["ar"])] + _src_errs(r["s32"], r)
    ehip = [rel_err(r["gr"], r["r64"], r["ar"])] + _src_errs(r["gs"], r)
    print("%s %s rel_err [g_ref, g_src, g_src per view ...]: fp32 oracle %s, HIP %s"
          % (name, metric, ["%.2e" % e for e in e32], ["%.2e" % e for e in ehip]))
    # the bound is one fp32 can meet: autograd of the oracle in fp32 meets it, per view too
    assert max(e32) <= TOL, e32
    assert ehip[0] <= TOL, ("g_ref", ehip[0])
    assert ehip[1] <= TOL, ("g_src", ehip[1])
    for v, e in enumerate(ehip[2:]):
        assert e <= TOL, ("g_src of view %d against that view's max" % v, e)
    if metric == "L1":   # the allowance is the exception, not the rule
        touched = (int((r["ar"] > 0).sum()) / r["ar"].numel(), int((r["as_"] > 0).sum()) / r["as_"].numel())
        print("%s L1 allowance touches %.4f %% of g_ref, %.4f %% of g_src" % (name, 100 * touched[0], 100 * touched[1]))
        assert max(touched) <= 1e-2, touched


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_texels_of_split_and_direct_pairs(dev, name, metric):
    """The texels that a pair with a direct plane or with several groups writes, against float64 under the same bound; the
    message names the pair and its groups, so a failure says which path broke.  (Other pairs add to these texels too: a
    failure in a box that several pairs share names each of them.)"""
    r = _result(dev, name, metric)
    pairs = _interesting(_groups(name))
    assert pairs, name
    failures = []
    for (i, v, ty, tx), gs in pairs.items():
        x_lo, x_hi, y_lo, y_hi = U.pair_box(gs)
        sl = (i, v, slice(None), slice(y_lo, y_hi + 1), slice(x_lo, x_hi + 1))
        allow = None if r["as_"] is None else r["as_"][sl]
        e = rel_err(r["gs"][sl], r["s64"][sl], allow, den=r["s64"][:, v].abs().max())
        if not e <= TOL:
            failures.append("item %d view %d tile (%d, %d): rel_err %.3e in x %d..%d y %d..%d; groups: %s"
                            % (i, v, ty, tx, e, x_lo, x_hi, y_lo, y_hi, U.describe(gs)))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_one_output_at_a_time(dev, name, metric):
    r = _result(dev, name, metric)
    gr, none, _ = hip_grads(r["d"], r["gup"], SIGMA, metric, want_src=False)
    assert none is None and torch.equal(gr, r["gr"])
    none, gs, _ = hip_grads(r["d"], r["gup"], SIGMA, metric, want_ref=False)
    assert none is None
    assert float((gs - r["gs"]).abs().max()) <= TOL_ORDER * float(r["gs"].abs().max())


@pytest.mark.gpu
def test_gradients_reproducible_on_case_a(dev):
    r = _result(dev, "A", "L2")
    gr, gs, _ = hip_grads(r["d"], r["gup"], SIGMA, "L2")
    assert torch.equal(gr, r["gr"])
    assert float((gs - r["gs"]).abs().max()) <= TOL_ORDER * float(r["gs"].abs().max())
