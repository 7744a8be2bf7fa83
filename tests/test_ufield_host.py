"""CPU only: keeps the reference of tests/util_ufield.py honest and checks the conditions the GPU suite (test_ufield_gpu.py)
relies on -- that the index restatement is grid_sample's, that the reference reproduces the oracle on every column of every
case, that the cases have qualifying pixels and no pixel on a threshold, and that each of seven plausible kernel mistakes
fails the comparison the GPU test makes on a case named here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pdepth_amd  # noqa: F401
from pdepth_amd import ops
from oracle import ref_cpu as O
from util import golden
import util_ufield as U


# ---- 1. the index restatement ------------------------------------------------------------------------------------------------
def _grid_sample_index(n, shift, axis):
    """Source index per destination index along `axis` (0: rows, 1: columns) of an n x 2 (2 x n) index image sampled through
    O._convert_flowfield's grid; -1 = padding."""
    shape = (n, 2) if axis == 0 else (2, n)
    idx = torch.arange(1, n + 1, dtype=torch.float32)
    img = (idx[:, None] if axis == 0 else idx[None, :]).expand(shape).reshape(1, 1, *shape).contiguous()
    flow = torch.zeros(1, shape[0], shape[1], 2)
    flow[..., 1 - axis] = shift                                   # (channel 0 is x, channel 1 is y)
    out = F.grid_sample(img, O._convert_flowfield(flow), mode="nearest", align_corners=False)[0, 0]
    line = out[:, 0] if axis == 0 else out[0, :]                  # (line 0 of the other axis: its own index is in the image)
    return line.long().numpy() - 1


def test_nearest_src_is_grid_sample_through_the_reference_grid():
    sizes = list(range(2, 401)) + [511, 512, 513, 640, 1024]
    n_checked = 0
    for n in sizes:
        for shift in (0.0, 0.5, -0.5, 1, 2, 2.5, -3, 5, 7, n + 3):
            want = _grid_sample_index(n, shift, 0)
            got = U.nearest_src(n, shift, True)
            assert np.array_equal(got, want), (n, shift)
            n_checked += 1
        if n % 37 == 0 or n > 500:                                # the columns go through the same function: a sample of sizes
            assert np.array_equal(U.nearest_src(n, 0.0, True), _grid_sample_index(n, 0.0, 1)), n
            assert np.array_equal(U.nearest_src(n, 2.0, True), _grid_sample_index(n, 2.0, 1)), n
    assert n_checked == 4040
    assert np.array_equal(U.nearest_src(7, 5.0, False), np.arange(7))
    # what the cases lean on: an even size loses its last index even unshifted, an odd one does not
    assert U.nearest_src(66, 0.0, True)[-1] == -1 and U.nearest_src(65, 0.0, True)[-1] == 64
    assert bool((U.nearest_src(2, 4.0, True) == -1).all())


# ---- 2. the reference against the oracle -------------------------------------------------------------------------------------
def _oracle_depth(c, bv_log):
    return U.cached(("odepth", c["name"], id(c["log"]), bv_log),
                    lambda: O.dpv_to_depthmap(U.volume(c, bv_log)[None], c["d_candi"], BV_log=bv_log)[0].numpy())


def _host_reference(c, v):
    return U.cached(("href", c["name"], v), lambda: U.reference(c, v, _oracle_depth(c, v[1])))


def _oracle(c, v):
    ang, bv_log, (mind, quash), mname = v
    m = c["masks"][mname]
    plane, dz = O.gen_ufield(U.volume(c, bv_log)[None], c["d_candi"], c["intr"], ang, c["z_start"], c["span"], BV_log=bv_log,
                             mask=None if m is None else m[None], mind=mind, quash_limit=quash)
    return plane[0].numpy(), dz[0].numpy()


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_reference_reproduces_the_oracle_on_every_column(name):
    """ufield_reference on the oracle's depth map against O.gen_ufield: depth_zero bit for bit, the NaN pattern of the plane,
    the plane within plane_bound(H) plus the same again for the oracle's own float32 sum.  No column is left out."""
    c = U.case(name)
    H, W = c["shape"][1:]
    worst, nan_cols = 0.0, {}
    for v in U.variants(name):
        plane, dz = _oracle(c, v)
        cmp = U.compare(plane, dz, _host_reference(c, v), H, bound_factor=2.0)
        assert U.matches(cmp), (name, U.variant_id(v), cmp)
        worst = max(worst, cmp["worst"])
        nan_cols[v] = np.isnan(plane).any(axis=0)
        assert np.array_equal(nan_cols[v], np.isnan(plane).all(axis=0))
        if v[3] == "columns_zeroed":                              # NaN in exactly the zeroed columns, besides those that are
            want = nan_cols[v[:3] + ("random",)].copy()           # empty under the mask they were zeroed in
            want[[0, W // 2]] = True
            assert np.array_equal(nan_cols[v], want), (name, U.variant_id(v))
        if U.degenerate(name, v):                                 # a shift beyond H: an all-NaN plane, a zero depth_zero
            assert not dz.any()
            # (probabilities, no minimum depth, no mask: the padding's depth 0 passes every test, the columns count H pixels
            #  of which none comes back through the inverse shift, and the plane is 0 / H)
            counted = not v[1] and v[2][0] == 0 and v[3] == "none"
            assert bool((plane == 0).all()) if counted else bool(np.isnan(plane).all())
    print("%s: %d variants, oracle's worst |f32 - f64| = %.3f of 2 plane_bound" % (name, len(U.variants(name)), worst))


def test_one_column_without_a_shift_is_legal_and_a_shifted_line_is_not():
    """W = 1 (or H = 1) with unc_ang = 0: the reference clones instead of sampling, nothing divides by size - 1.  With a shift
    convert_flowfield divides by zero for H = 1 or W = 1, and so does ops.ufield, before it looks at anything else."""
    for c in (U.one_column_case(), U.one_row_case()):
        for v in [(0, bv, br, m) for bv in (True, False) for br in U.BRANCHES for m in ("none", "random")]:
            plane, dz = _oracle(c, v)
            assert U.matches(U.compare(plane, dz, _host_reference(c, v), c["shape"][1], bound_factor=2.0)), U.variant_id(v)
    for shape in ((1, 4, 1, 8), (2, 4, 8, 1), (1, 4, 1, 1)):
        with pytest.raises(ZeroDivisionError):
            O.gen_ufield(torch.zeros(1, *shape[1:]), np.ones(4), torch.eye(3), 5, 0.0, 1.0)
        for ang in (5, -3, 0.5):
            with pytest.raises(ZeroDivisionError):
                ops.ufield(torch.zeros(shape), np.ones(4), torch.eye(3).expand(shape[0], 3, 3), unc_ang=ang)


# ---- 3. the reference against the fixtures -----------------------------------------------------------------------------------
def _stable_columns(vol, d_candi, intr, okw):
    """test_round2_rows.py::test_hip_ufield's rule: the columns whose plane does not change when the depth map moves by
    ~5e-4.  Needed here only: the fixtures' depth map was summed on another machine."""
    base, _ = O.gen_ufield(vol, d_candi, intr, **okw)
    stable = np.ones(base.shape[2], dtype=bool)
    for eps in (-2e-5, 2e-5):
        p2, _ = O.gen_ufield(vol, d_candi * (1.0 + eps), intr, **okw)
        stable &= np.isclose(p2.numpy(), base.numpy(), rtol=1e-6, atol=1e-9, equal_nan=True).all(axis=(0, 1))
    return stable


def _against_fixture(tag, vol, d_candi, intr, mask, bv_log, okw, want_plane, want_dz):
    stable = _stable_columns(vol, d_candi, intr, dict(okw, BV_log=bv_log, mask=mask))
    assert stable.mean() > 0.8, tag
    depth = O.dpv_to_depthmap(vol, d_candi, BV_log=bv_log)[0].numpy()
    ref = U.ufield_reference(vol[0].numpy(), d_candi, intr.numpy(), None if mask is None else mask[0].numpy(), bv_log,
                             okw["unc_ang"], okw["unc_shift"], okw["unc_shift"] + okw["unc_span"], okw["mind"], okw["quash_limit"],
                             depth)
    H = vol.shape[2]
    cmp = U.compare(want_plane[0], ref["depth_zero"], ref, H, bound_factor=2.0, skip_columns=~stable)
    assert cmp["nan_diff"] == 0 and cmp["over"] == 0, (tag, cmp)
    if want_dz is not None:
        np.testing.assert_allclose(ref["depth_zero"][:, stable], want_dz[0][:, stable], rtol=0, atol=1e-4, err_msg=tag)
    return int(stable.sum())


def test_reference_matches_the_reference_fixtures():
    """g14 (cfgx branch, shifts 0 and nonzero, with and without mask) and g19 (both dataset branches), which the reference
    itself made: the plane on the stable columns within 2 plane_bound, the NaN pattern, the masked depth to 1e-4."""
    g = golden("g14_ufield.npz")
    intr = torch.from_numpy(g["intr"])
    checked = 0
    for tag in ("a", "b"):
        ang, shift, span = g[tag + "_cfgx"]
        okw = dict(unc_ang=int(ang), unc_shift=float(shift), unc_span=float(span), mind=3.0, quash_limit=True)
        logdpv, mask = torch.from_numpy(g[tag + "_logdpv"]), torch.from_numpy(g[tag + "_mask"])
        checked += _against_fixture("g14/" + tag + "/log", logdpv, g["d_candi"], intr, None, True, okw, g[tag + "_plane_log"],
                                    g[tag + "_depthzero_log"])
        checked += _against_fixture("g14/" + tag + "/prob+mask", torch.exp(logdpv), g["d_candi"], intr, mask, False, okw,
                                    g[tag + "_plane_prob_masked"], g[tag + "_depthzero_prob_masked"])
    g = golden("g19_unc_field.npz")
    intr = torch.from_numpy(g["intr"])[0]
    for tag in ("kitti", "ilim"):
        okw = dict(O.UFIELD_DATASETS[tag])
        checked += _against_fixture("g19/" + tag + "/truth", torch.from_numpy(g[tag + "_truth_dpv"]), g["d_candi"], intr,
                                    torch.from_numpy(g[tag + "_mask"]), False, okw, g[tag + "_field_truth"], None)
        checked += _against_fixture("g19/" + tag + "/pred", torch.from_numpy(g[tag + "_pred_logdpv"]), g["d_candi"], intr, None,
                                    True, okw, g[tag + "_field_pred"], g[tag + "_debugmap"])
    assert checked > 400


# ---- 4. conditions on the inputs ---------------------------------------------------------------------------------------------
def test_cases_have_qualifying_pixels_and_none_on_a_threshold():
    """Per non-degenerate variant the share of qualifying pixels, taken over the columns the mask does not zero on purpose,
    lies in [1 %, 90 %].  (A variant is degenerate when the shift reaches H or the mask zeroes every column: two_columns
    with its columns 0 and 1 zeroed.)  Under quash a column keeps one +-1 m window around its nearest surface however tall
    the image is, so its yield is a number of pixels per column, not a share of H: there the floor is the smaller of 1 % and
    one pixel per column on the average -- what 1 % asks of a 100-row image (model_rows: 256 rows, 1.9 pixels per column,
    0.7 %).  Over all cases fewer than 1 % of the columns hold a pixel within 2 ulp of a threshold (none does)."""
    cols = near_cols = 0
    for name in U.CASE_NAMES:
        c = U.case(name)
        H, W = c["shape"][1:]
        lo, hi = 1.0, 0.0
        for v in U.variants(name):
            ref = _host_reference(c, v)
            cols += W
            near_cols += int(ref["near"].any(axis=0).sum())
            live = np.ones(W, dtype=bool)
            if v[3] == "columns_zeroed":
                live[[0, W // 2]] = False
            if U.degenerate(name, v) or not live.any():
                continue
            share = float(ref["zm"][:, live].mean())
            lo, hi = min(lo, share), max(hi, share)
            floor = min(0.01, 1.0 / H) if v[2][1] else 0.01
            assert floor <= share <= 0.90, (name, U.variant_id(v), share)
        print("%s: qualifying pixels %.1f %% .. %.1f %%" % (name, 100 * lo, 100 * hi))
    print("columns with a pixel on a threshold: %d of %d" % (near_cols, cols))
    assert near_cols < 0.01 * cols


def test_rows_shifted_in_from_outside_qualify_when_the_candidates_sum_below_99():
    c = U.case("oob_depth_in_range")
    H = c["shape"][1]
    assert float(U.oob_depth(c["d_candi"], True)) == 33.0
    for v, rows in (((5, True, U.BRANCHES[0], "none"), range(0, 5)), ((5, True, U.BRANCHES[1], "none"), range(0, 5))):
        sy = U.nearest_src(H, v[0], True)
        assert np.array_equal(np.flatnonzero(sy < 0), np.array(rows))
        assert _host_reference(c, v)["zm"][sy < 0].sum() >= 1
    # everywhere else the depth from outside is beyond the range test and no such row can qualify
    for name in ("scalar_ragged", "model_rows"):
        assert float(U.oob_depth(U.case(name)["d_candi"], True)) > 99.0


# ---- 5. the cases discriminate -----------------------------------------------------------------------------------------------
def _caught(c, v, wrong=None, **kw):
    """Does the comparison of the GPU test (float32 plane, depth_zero against the reference on the same depth map) tell the
    wrong reference from the right one?"""
    depth = _oracle_depth(c, v[1])
    right = U.reference(c, v, depth, mask=kw.get("mask")) if kw else _host_reference(c, v)
    bad = U.reference(c, v, depth, wrong=wrong, **kw)
    return not U.matches(U.compare(bad["plane"].astype(np.float32), bad["depth_zero"], right, c["shape"][1]))


def _shifted(name):
    return [v for v in U.variants(name) if v[0] != 0 and not U.degenerate(name, v)]


# wrong reference -> the cases that must catch it
CATCHERS = {
    "back_shift_plus": ("scalar_even", "model_rows"),
    "sx_identity": ("scalar_even", "vec4_odd_planes", "tall_narrow"),
    "last_row_dropped": ("scalar_even", "vec4_odd_planes"),
    "last_segment_dropped": ("scalar_even", "tall_narrow", "vec4_short"),
    "oob_zero": ("oob_depth_in_range", "vec4_wide_short"),
    "quash_unmasked": ("scalar_ragged", "vec4_odd_planes"),
}


@pytest.mark.parametrize("wrong", U.WRONG)
def test_a_wrong_reference_fails_the_comparison_on_a_named_case(wrong):
    for name in CATCHERS[wrong]:
        c = U.case(name)
        hits = [v for v in U.variants(name) if _caught(c, v, wrong)]
        print("%s caught by %s in %d of %d variants" % (wrong, name, len(hits), len(U.variants(name))))
        assert hits, (wrong, name)
        if wrong in ("back_shift_plus", "sx_identity"):
            # both are invisible without a shift (the reference clones), so it is the shifted variants that must catch them, each
            # of them; a missing column gather also escapes an odd width, whose grid keeps every column
            assert {U.variant_id(v) for v in _shifted(name)} <= {U.variant_id(v) for v in hits}, (wrong, name)
            assert not any(v[0] == 0 for v in hits)
        if wrong == "last_segment_dropped" and name != "vec4_short":
            assert len(hits) == len(U.variants(name))             # tall images: every variant has a pixel in the last eighth
        if wrong == "oob_zero":
            assert all(v[1] and v[0] != 0 for v in hits)          # only a log-DPV pads with ones
    if wrong == "sx_identity":
        c = U.case("scalar_ragged")                               # W = 65
        assert not any(_caught(c, v, wrong) for v in U.variants("scalar_ragged"))


def test_another_items_intrinsics_fail_the_comparison():
    """Item 1 of the B = 3 calls evaluated with item 0's cy and fy (an unscaled `b * 9`): caught by scalar_ragged and
    vec4_odd_planes in both calls the GPU test makes, by tall_narrow in the unquashed one (under quash the nearest surface of
    its four columns lies inside both bands)."""
    for name in U.BATCH_CASES:
        items = U.batch_items(name)
        assert not torch.equal(items[0]["intr"], items[1]["intr"]) and not torch.equal(items[0]["log"], items[1]["log"])
        hits = [_caught(items[1], v, mask=items[1]["mask"], intr=items[0]["intr"]) for v in U.BATCH_VARIANTS]
        assert hits[1], name
        if name != "tall_narrow":
            assert hits[0], name
