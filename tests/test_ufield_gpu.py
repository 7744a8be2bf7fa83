"""pdepth_ufield_f32 (csrc/ufield.hip: the mask and quash kernel, the scalar and the vec4 collapse) against the reference of
tests/util_ufield.py on every column of every case: no column is left out because "a pixel near a threshold may flip".

The masks are comparisons of float32 values that IEEE operations derive from the depth map, and that depth map is bit for bit
what ops.dpv_expect returns on the same tensor (launch_ufield calls the same launch_dpv_expect).  So the reference, handed
that map, decides every mask exactly: depth_zero must be bit-equal, the NaN pattern of the plane equal, and the plane within
plane_bound(H) = (ceil(H / 8) + 24) 2^-24 of the float64 sum (derived in util_ufield.plane_bound).  test_ufield_host.py shows
the reference reproducing the oracle the same way, and seven wrong kernels failing this comparison on cases named there.

  case                D,H,W        exercises
  two_columns         5,9,2        smallest width; even W loses its last column when shifted
  two_rows            7,2,13       H < 8: empty row segments; a shift beyond H
  scalar_ragged       33,30,65     scalar collapse, second 64-column block holds one column, D % 4 = 1
  scalar_even         8,257,66     scalar, even W, second trip of the mask kernel's 256-row loop
  vec4_odd_planes     9,33,260     vec4, last plane pair half empty, second 256-column block holds one quad
  vec4_wide_short     2,16,256     vec4, exactly one block, exactly one row per segment
  vec4_short          64,12,132    vec4 with 8 < H < 16: empty segments
  tall_narrow         4,513,4      third trip of the mask loop, one quad
  oob_depth_in_range  3,300,8      sum(d) = 33 < 99: rows shifted in from outside qualify
  d_over_128          130,12,40    inner expectation on the D > 128 kernel
  model_rows          64,256,68    the model's row count at the narrowest vec4 width with an odd quad count
  unaligned           8,20,64      volume one float into a flat buffer: scalar collapse and scalar expectation
Each with unc_ang 0, 5, -3 (two_rows also H + 2, scalar_ragged also 2.5), as log-DPV and as probabilities, on both dataset
branches (min depth 3 + quash, 0 without), with no mask, a random one and one with two columns zeroed.

Measured on an MI355X (printed by the tests, -s):
  worst |got - f64| in units of plane_bound, over a case's variants: two_columns 0.039, two_rows 0.037, scalar_ragged 0.156,
    scalar_even 0.086, vec4_odd_planes 0.136, vec4_wide_short 0.120, vec4_short 0.132, tall_narrow 0.048,
    oob_depth_in_range 0.073, d_over_128 0.134, model_rows 0.094, unaligned 0.125.  (The oracle's own float32 sum on the host:
    0.03 ... 0.19 of the same unit.)  The B = 3 calls: scalar_ragged 0.062 / 0.121, vec4_odd_planes 0.074 / 0.136,
    tall_narrow 0.021 / 0.048 (quashed log-DPV / unquashed probabilities).
  inner depth map against the float64 expectation: 9e-7 ... 1.0e-5 m (d_over_128), bound 1e-4 m.
  depth_zero bit-equal and the NaN pattern equal in all 457 + 16 single-item calls and all 18 batch items; skipped columns: 0
    of 36209 (and the host test finds no pixel within 2 ulp of a threshold in any case).  No mask decision failed to
    reproduce, and no kernel bug was found.
  unaligned against aligned: the scalar and the wave-layout expectation differ in the last bits of 3926 depth pixels over the
    36 variants (of 46080), so depth_zero is NOT bit-equal between the two calls; the masks are.
"""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops, synth
from pdepth_amd.utils import img_utils
from util import DEPTH_ATOL
import util_ufield as U

pytestmark = pytest.mark.gpu

# Columns left out of a comparison because numpy cannot follow a correct kernel there.  None is: the count is kept so that
# the cap of the host test (fewer than 1 % of the columns hold a pixel on a threshold) has something to hold.
SKIPPED_COLUMNS = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _upload(name, vol, dev):
    """[1,D,H,W] on the device; for `unaligned` a contiguous view one float into a flat buffer."""
    if name != "unaligned":
        return vol[None].to(dev)
    flat = torch.empty(vol.numel() + 1, device=dev)
    flat[1:].copy_(vol.reshape(-1))
    out = flat[1:].view(1, *vol.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _call(c, v, dev, vol_dev, mask=None, intr=None, d_candi=None):
    ang, bv_log, (mind, quash), mname = v
    m = c["masks"][mname] if mask is None else mask
    if m is not None and m.dim() == 2:
        m = m[None]
    intr = c["intr"][None] if intr is None else intr
    plane, dz = ops.ufield(vol_dev, c["d_candi"] if d_candi is None else d_candi, intr.to(dev), None if m is None else m.to(dev),
                           BV_log=bv_log, unc_ang=ang, z_start=c["z_start"], z_end=c["z_end"], min_depth=mind, quash=quash)
    return plane.cpu(), dz.cpu()


def _depth(c, bv_log, vol_dev, name):
    """ops.dpv_expect on the very tensor of the ufield call, within DEPTH_ATOL of the float64 expectation."""
    depth = ops.dpv_expect(vol_dev, c["d_candi"], BV_log=bv_log).cpu().numpy()
    want = U.depth64(U.volume(c, bv_log).numpy(), c["d_candi"], bv_log)
    err = float(np.abs(depth[0].astype(np.float64) - want).max())
    assert err <= DEPTH_ATOL, "%s: inner depth map %.3e from float64" % (name, err)
    return depth[0], err


def _check(tag, plane, dz, ref, H):
    cmp = U.compare(plane.numpy(), dz.numpy(), ref, H)
    assert cmp["dz_diff"] == 0, "%s: depth_zero differs in %d pixels (columns %s)" % (tag, cmp["dz_diff"], cmp["bad_columns"][:8])
    assert cmp["nan_diff"] == 0, "%s: NaN pattern differs in columns %s" % (tag, cmp["bad_columns"][:8])
    assert cmp["over"] == 0, "%s: plane %.2f plane_bound off in columns %s" % (tag, cmp["worst"], cmp["bad_columns"][:8])
    return cmp["worst"]


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_ufield_against_the_reference_on_every_column(dev, name):
    c = U.case(name)
    D, H, W = c["shape"]
    vols = {bv: _upload(name, U.volume(c, bv), dev) for bv in (True, False)}
    depth = {bv: _depth(c, bv, vols[bv], name) for bv in (True, False)}
    worst = 0.0
    for v in U.variants(name):
        plane, dz = _call(c, v, dev, vols[v[1]])
        assert plane.shape == (1, D, W) and dz.shape == (1, H, W)
        worst = max(worst, _check(name + " " + U.variant_id(v), plane[0], dz[0], U.reference(c, v, depth[v[1]][0]), H))
    print("%s: %d variants, worst |got - f64| = %.3f plane_bound, inner depth %.1e / %.1e m from float64, skipped columns %d"
          % (name, len(U.variants(name)), worst, depth[True][1], depth[False][1], SKIPPED_COLUMNS))
    assert SKIPPED_COLUMNS == 0


@pytest.mark.parametrize("name", U.BATCH_CASES)
def test_ufield_batch_of_three(dev, name):
    """One B = 3 call (a quashed log-DPV one, and an unquashed one on probabilities): three seeds of the case, cy shifted by
    0, +1.7, -2.4 rows and fy scaled by 1, 0.8, 1.3, masks random, all ones, all zero.  Bit for bit the three B = 1 calls on
    the slices, each item within the bounds against its own reference; the masked-out item is an all-NaN plane and a zero
    depth_zero and leaves its neighbours alone."""
    items = U.batch_items(name)
    D, H, W = items[0]["shape"]
    intr = torch.stack([it["intr"] for it in items])
    mask = torch.stack([it["mask"] for it in items])
    assert bool(mask[1].all()) and not bool(mask[2].any())
    for v in U.BATCH_VARIANTS:
        vol = torch.stack([U.volume(it, v[1]) for it in items]).to(dev)
        depth = ops.dpv_expect(vol, items[0]["d_candi"], BV_log=v[1]).cpu().numpy()
        plane, dz = _call(items[0], v, dev, vol, mask=mask, intr=intr)
        assert plane.shape == (3, D, W) and dz.shape == (3, H, W)
        worst = 0.0
        for b, it in enumerate(items):
            p1, d1 = _call(it, v, dev, vol[b:b + 1], mask=mask[b:b + 1], intr=intr[b:b + 1])
            assert torch.equal(torch.nan_to_num(p1[0], nan=-1.0), torch.nan_to_num(plane[b], nan=-1.0)), (name, b)
            assert torch.equal(d1[0], dz[b]), (name, b)
            ref = U.reference(it, v, depth[b], mask=it["mask"])
            worst = max(worst, _check("%s item %d %s" % (name, b, U.variant_id(v)), plane[b], dz[b], ref, H))
        assert bool(torch.isnan(plane[2]).all()) and not bool(dz[2].any())
        assert bool(torch.isfinite(plane[1]).any()) and bool(dz[1].any()) and bool(dz[0].any())
        print("%s B=3 %s: worst |got - f64| = %.3f plane_bound" % (name, U.variant_id(v), worst))


def test_scalar_and_vec4_collapse_agree(dev):
    """`unaligned` and the same values in an aligned tensor: each within plane_bound of its reference with a bit-equal
    depth_zero.  The two calls also run different expectation kernels, whose depth maps differ in the last bits, so between
    the two calls depth_zero is equal in its zero pattern (the same masks) and to 2 DEPTH_ATOL in value, and the planes are
    within 2 plane_bound of each other."""
    c = U.case("unaligned")
    D, H, W = c["shape"]
    differing = 0
    for v in U.variants("unaligned"):
        out = {}
        for how in ("unaligned", "aligned"):
            vol = _upload(how, U.volume(c, v[1]), dev)
            assert (vol.data_ptr() % 16 == 0) == (how == "aligned")
            depth = ops.dpv_expect(vol, c["d_candi"], BV_log=v[1]).cpu().numpy()[0]
            plane, dz = _call(c, v, dev, vol)
            ref = U.reference(c, v, depth)
            _check("%s %s" % (how, U.variant_id(v)), plane[0], dz[0], ref, H)
            out[how] = (plane[0].double().numpy(), dz[0].numpy(), ref)
        (pu, du, ru), (pa, da, ra) = out["unaligned"], out["aligned"]
        assert np.array_equal(ru["zm"], ra["zm"]) and np.array_equal(du != 0, da != 0)
        assert float(np.abs(du - da).max()) <= 2 * DEPTH_ATOL
        assert np.array_equal(np.isnan(pu), np.isnan(pa))
        fin = ~np.isnan(pu)
        assert bool((np.abs(pu - pa)[fin] <= 2 * U.plane_bound(H) * np.abs(pa[fin]) + U.ABS_BOUND).all())
        differing += int((du != da).sum())
    print("unaligned against aligned: %d pixels of depth_zero differ in the last bits over %d variants" % (differing, len(U.variants("unaligned"))))


def test_candidates_on_the_device(dev):
    """d_candi as a device tensor: the out-of-bounds depth is read back from the device (oob_depth_in_range, where it decides
    masks).  Bit for bit the host-array call."""
    c = U.case("oob_depth_in_range")
    for bv in (True, False):
        vol = U.volume(c, bv)[None].to(dev)
        for br in U.BRANCHES:
            v = (5, bv, br, "random")
            want = _call(c, v, dev, vol)
            got = _call(c, v, dev, vol, d_candi=torch.tensor(c["d_candi"], dtype=torch.float32, device=dev))
            got64 = _call(c, v, dev, vol, d_candi=torch.tensor(c["d_candi"], dtype=torch.float64, device=dev))
            for g in (got, got64):
                assert torch.equal(torch.nan_to_num(g[0], nan=-1.0), torch.nan_to_num(want[0], nan=-1.0)) and torch.equal(g[1], want[1])
            assert bool(torch.isfinite(want[0]).any())


def test_gen_ufield_wrapper_equals_the_batched_call(dev):
    """img_utils.gen_ufield on the item is ops.ufield bit for bit on all three parameter branches; normalize=True is the
    min/max formula applied to that plane."""
    c = U.case("scalar_ragged")
    vol, intr = c["log"][None].to(dev), c["intr"].to(dev)
    mask = c["masks"]["random"][None].to(dev)
    cfgx = {"unc_ang": 5, "unc_shift": c["z_start"], "unc_span": c["span"]}
    kitti, ilim = (synth.Cfg({"data": {"dataset_path": p}}) for p in ("/data/kitti/raw", "/data/ilim/set1"))
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    finite = 0
    for kw, okw in ((dict(cfgx=cfgx), dict(unc_ang=5, z_start=c["z_start"], z_end=c["z_start"] + c["span"], min_depth=3.0, quash=True)),
                    (dict(cfg=kitti), dict(unc_ang=5, z_start=0.6, z_end=0.6 + 0.3, min_depth=0.0, quash=False)),
                    (dict(cfg=ilim), dict(unc_ang=0, z_start=1.0, z_end=1.0 + 0.3, min_depth=3.0, quash=True))):
        for m in (None, mask):
            plane, dz = img_utils.gen_ufield(vol, c["d_candi"], intr, mask=m, BV_log=True, **kw)
            wp, wd = ops.ufield(vol, c["d_candi"], intr[None], m, BV_log=True, **okw)
            assert same(plane, wp) and torch.equal(dz, wd)
            norm, nd = img_utils.gen_ufield(vol, c["d_candi"], intr, mask=m, BV_log=True, normalize=True, **kw)
            lo, hi = wp.min(1)[0], wp.max(1)[0]
            assert same(norm, (wp - lo) / (hi - lo)) and torch.equal(nd, wd)
            finite += int(torch.isfinite(wp).sum())
    assert finite > 0


def test_single_column_or_row_without_a_shift(dev):
    """W = 1 and H = 1 are legal with unc_ang = 0 (nothing is sampled); with a shift the call raises before any launch, as
    the reference's grid construction does (test_ufield_host.py pins the exception)."""
    for c in (U.one_column_case(), U.one_row_case()):
        D, H, W = c["shape"]
        for bv in (True, False):
            vol = U.volume(c, bv)[None].to(dev)
            depth = ops.dpv_expect(vol, c["d_candi"], BV_log=bv).cpu().numpy()[0]
            for br in U.BRANCHES:
                for m in ("none", "random"):
                    v = (0, bv, br, m)
                    plane, dz = _call(c, v, dev, vol)
                    assert plane.shape == (1, D, W) and dz.shape == (1, H, W)
                    _check(c["name"] + " " + U.variant_id(v), plane[0], dz[0], U.reference(c, v, depth), H)
        with pytest.raises(ZeroDivisionError):
            _call(c, (5, True, U.BRANCHES[0], "none"), dev, vol)
