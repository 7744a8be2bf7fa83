"""ops.dpv_soft_ce (csrc/loss.hip) on every kernel path against the float64 restatement of tests/util_soft_ce.py: every pixel's
ce, every item's loss and count, the depth map and every element of g_logp inside the a-priori bounds derived there, non-finite
elements by class (NaN, +inf, -inf), with no absolute tolerance beyond the stated floor of a few 2^-126.  Every case asserts the
path it reaches through util_soft_ce.which_path before it calls the op, and every test the set of paths its cases reached.

  per-pixel forward   ce is observed through probe items: the item is repeated B = H W times and item b's mask is 1 at pixel b
                      alone, so loss[b] = ce[b] and count[b] = 1 (blockIdx.y runs to 260).  Every pixel at 9 x 12 (108 pixels: less
                      than a workgroup) and 13 x 20 (260: the second workgroup holds one live quad and three dead waves), D in
                      {1, 3, 4, 5, 32, 33, 64, 65, 100, 127, 128} (vec8, vec16, vec32: the first and a ragged D of each), both label
                      sources; the scalar kernels at 7 x 9, 1 x 257 (two workgroups), D in {129, 130} at 8 x 8 and at D = 64, 9 x 12
                      with logp, the label, depth_gt or the mask one float into its buffer
  loss and count      B = 3, the four mask kinds (binary; values 0.5 and 2.0; all-zero on one item; none), count exact
  backward            g_loss only, g_depth only, both; both label sources; masks with 0.5 and 2.0; every D above at both shapes
                      and the scalar reasons, g_depth one float into its buffer among them
  from-depth edges    variance 0.01 at D = 8 (-1 pixels inside the range: the -1 set, read off the sign of g_logp, equals the
                      reference's exactly), pow in {1, 2, 3, 0.5}, depth_gt on a candidate, midway, below d_0, above d_(D-1), NaN, +inf
  non-finite logp     -inf where the label is > 0 (ce = +inf), -inf where a label entry is exactly 0 (NaN), both again behind a zero mask
  kept from the old suite at small shapes: depth is bit-equal to ops.dpv_expect(BV_log=True), two calls give equal bits.

test_soft_ce_host.py shows float32 emulations of both summation orders inside the bounds (ce 0.62, depth 0.44, loss 0.07, g_logp
0.61 of them at the worst) and twelve planted mistakes at least 3.9e+03 times outside.

Measured on an MI355X (printed by the tests, -s), worst err / bound per path over all cases of this file, label | from depth:
            ce              depth           loss            g_logp: g_loss only, g_depth only, both
  vec8      0.118 | 0.101   0.380 | 0.375   0.082 | 0.016   0.604 | 0.285   0.452 | 0.452   0.608 | 0.536
  vec16     0.107 | 0.065   0.166 | 0.173   0.040 | 0.027   0.568 | 0.398   0.456 | 0.485   0.566 | 0.513
  vec32     0.148 | 0.052   0.136 | 0.150   0.045 | 0.019   0.545 | 0.238   0.501 | 0.483   0.589 | 0.510
  scalar    0.127 | 0.081   0.327 | 0.284   0.060 | 0.047   0.654 | 0.278   0.474 | 0.487   0.568 | 0.522
The gradient of the label form is a chain of three products held to gamma_3: a worst case of 0.65 is what three roundings give.
ce sits lower at large D, as the correlation suite's ratios do (the bound grows like n u A, the error of a sum of mixed
roundings like sqrt(n) u A), and the from-depth ce lower still: its bound carries expf's error at twice the measured worst and the
rounding of arg magnified by arg on every plane, and the weighted mean cancels most of both.  No ratio is above 1, the -1 sets
are the reference's, every non-finite element has the reference's class: no defect was found in the arithmetic of any kernel.
Against a copy of the library with three mistakes planted in csrc/loss.hip (the last plane dropped on the vec4 forward when
D % 4 != 0, the coefficient without the mask's value, pow ignored) 27 of the 35 tests fail.
"""
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native as N
from pdepth_amd import ops
import util_soft_ce as U

pytestmark = pytest.mark.gpu
FORMS = ("label", "depth")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


class _Worst:
    """Worst err / bound per (path, label source, output), with the case that gave it."""

    def __init__(self):
        self.top = {}

    def note(self, path, form, name, got, ref, E, case):
        w = U.worst(got, ref, E)
        key = (path, form, name)
        if w > self.top.get(key, (-1.0, None))[0]:
            self.top[key] = (w, case)
        if not w <= 1.0:
            r = U.ratio(got, ref, E).flatten()
            i = int(r.argmax())
            print("OVER THE BOUND %s %s %s %s: ratio %.3g at flat index %d: got %r want %r bound %r" % (
                path, form, name, case, w, i, float(got.detach().cpu().double().flatten()[i]), float(ref.flatten()[i]),
                float(E.flatten()[i])))

    def reached(self):
        return {(p, f) for p, f, _ in self.top}

    def report(self, tag):
        for (path, form, name), (w, case) in sorted(self.top.items()):
            print("%s: %-6s %-5s %-6s worst err / bound = %.3f  %s" % (tag, path, form, name, w, case))
        over = {k: v for k, v in self.top.items() if not v[0] <= 1.0}
        assert not over, (tag, over)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _one_float_in(t):
    """The same values, contiguous, one float into a larger buffer: the pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _to_dev(c, dev, off=None, repeat=None):
    """The tensors of a case on the device as the binding will pass them (contiguous float32; `repeat`: the one item B times);
    `off` names the operand that sits one float into its buffer."""
    d = {}
    for k in ("logp", "label", "depth_gt", "mask", "g_loss", "g_depth", "dc"):
        t = c[k]
        if t is None:
            d[k] = None
            continue
        t = t.to(dev)
        if repeat and k in ("logp", "label", "depth_gt"):
            t = t.expand(repeat, *t.shape[1:])
        t = t.contiguous()
        assert t.data_ptr() % 16 == 0
        d[k] = _one_float_in(t) if off == k else t
    assert off is None or d[off] is not None
    return d


def _src(c, d):
    return dict(label=d["label"], depth_gt=d["depth_gt"], variance=c["variance"] if d["depth_gt"] is not None else None, pow=c["pow"])


def _forward(c, d, shape, expect, want_depth=True):
    path = U.which_path(shape, [d["logp"], d["label"], d["depth_gt"], d["mask"]])
    assert path == expect, (shape, path, expect)
    return N.dpv_soft_ce(d["logp"], d["dc"], mask=d["mask"], want_depth=want_depth, **_src(c, d))


def _backward(c, d, shape, count, grads, expect):
    gl = d["g_loss"] if grads in ("both", "loss") else None
    gd = d["g_depth"] if grads in ("both", "depth") else None
    path = U.which_path(shape, [d["logp"], d["label"], d["depth_gt"], d["mask"], gd])
    assert path == expect, (shape, grads, path, expect)
    return N.dpv_soft_ce_backward(d["logp"], d["dc"], count, mask=d["mask"], g_loss=gl, g_depth=gd, **_src(c, d))


def _vec(D):
    return U.VEC[U.planes_per_lane(D)]


# ---- per-pixel forward ----------------------------------------------------------------------------------------------------------
def _probe(rec, dev, D, hw, form, seed, expect, var=0.3, pw=2.0, off=None, family=None):
    """Every pixel's ce of one item through H W probe items."""
    H, W = hw
    HW = H * W
    family = family or U.VOLUMES[seed % 3]
    c = U.make_case(family, form, (1, D, H, W), seed, "none", var, pw)
    r = U.case_reference(c, grads=None)
    E = U.probe_bound(r, U.bound(r, expect)["ce"], expect)
    c["mask"] = torch.eye(HW).view(HW, H, W)
    d = _to_dev(c, dev, off=off, repeat=HW)
    loss, count, depth = _forward(c, d, (HW, D, H, W), expect)
    case = "%dx%dx%d %s %s var %g pow %g%s" % (D, H, W, form, family, var, pw, " %s off" % off if off else "")
    assert bool((count == 1).all()), case
    rec.note(expect, form, "ce", loss.view(1, H, W), r["ce"], E, case)
    assert _bits(depth[0]).equal(_bits(depth[HW - 1])), case
    rec.note(expect, form, "depth", depth[HW - 1:], r["depth"], U.bound(r, expect)["depth"], case)
    return r, c


@pytest.mark.parametrize("D", U.PROBE_D)
def test_every_pixel_on_the_vec4_kernels(dev, D):
    rec = _Worst()
    for i, hw in enumerate(U.PROBE_HW):
        for j, form in enumerate(FORMS):
            _probe(rec, dev, D, hw, form, 6000 + 4 * D + 2 * i + j, _vec(D))
    assert rec.reached() == {(_vec(D), f) for f in FORMS}
    rec.report("probes, D = %d" % D)


def test_every_pixel_on_the_scalar_kernels(dev):
    rec = _Worst()
    n = 0
    for hw in U.SCALAR_HW:            # H W % 4 != 0
        for D in (1, 5, 64):
            for form in FORMS:
                _probe(rec, dev, D, hw, form, 6100 + n, U.SCALAR)
                n += 1
    for D in U.SCALAR_D:              # D > 128
        for form in FORMS:
            _probe(rec, dev, D, (8, 8), form, 6100 + n, U.SCALAR)
            n += 1
    assert _vec(64) == U.which_path((108, 64, 9, 12), [])   # a pointer that is not 16-byte aligned, each operand in turn
    for form, offs in (("label", ("logp", "label", "mask")), ("depth", ("logp", "depth_gt", "mask"))):
        for off in offs:
            _probe(rec, dev, 64, (9, 12), form, 6100 + n, U.SCALAR, off=off)
            n += 1
    assert rec.reached() == {(U.SCALAR, f) for f in FORMS}
    rec.report("probes, scalar")


# ---- loss and count ---------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((3, 5, 9, 12), (3, 64, 13, 20), (3, 100, 13, 20), (3, 20, 7, 9), (3, 129, 8, 8))


@pytest.mark.parametrize("mask_kind", U.MASKS)
def test_loss_and_count(dev, mask_kind):
    rec = _Worst()
    for i, shape in enumerate(LOSS_SHAPES):
        B, D, H, W = shape
        expect = _vec(D) if (H * W) % 4 == 0 and D <= 128 else U.SCALAR
        for j, form in enumerate(FORMS):
            c = U.make_case(U.VOLUMES[(i + j) % 3], form, shape, 6200 + 2 * i + j, mask_kind)
            r = U.case_reference(c, grads=None)
            E = U.bound(r, expect)
            d = _to_dev(c, dev)
            loss, count, depth = _forward(c, d, shape, expect)
            case = "%s %s mask %s" % ("x".join(map(str, shape)), form, mask_kind)
            assert torch.equal(count.cpu().double(), r["count"]), case
            rec.note(expect, form, "loss", loss, r["loss"], E["loss"], case)
            rec.note(expect, form, "depth", depth, r["depth"], E["depth"], case)
            if mask_kind == "zero_item":
                assert float(r["count"][B - 1]) == 0.0 and float(loss[B - 1]) == 0.0, case
    assert {p for p, _ in rec.reached()} == {"vec8", "vec16", "vec32", U.SCALAR}
    rec.report("loss, mask %s" % mask_kind)


# ---- backward ---------------------------------------------------------------------------------------------------------------------
GRADS = ("loss", "depth", "both")


def _grad_case(rec, dev, shape, form, seed, expect, mask_kind, var=0.3, pw=2.0, off=None, family=None, consistency=False):
    B, D, H, W = shape
    c = U.make_case(family or U.VOLUMES[seed % 3], form, shape, seed, mask_kind, var, pw)
    d = _to_dev(c, dev, off=off)
    fwd_expect = U.SCALAR if off not in (None, "g_depth") else expect if off is None else _vec(D)
    loss, count, depth = _forward(c, d, shape, fwd_expect)
    case = "%s %s mask %s var %g pow %g%s" % ("x".join(map(str, shape)), form, mask_kind, var, pw, " %s off" % off if off else "")
    out = {}
    for grads in GRADS:
        r = U.case_reference(c, grads=grads)
        E = U.bound(r, expect)
        if grads == "loss":
            assert torch.equal(count.cpu().double(), r["count"]), case
            rec.note(fwd_expect, form, "loss", loss, r["loss"], U.bound(r, fwd_expect)["loss"], case)
        want = expect if (off != "g_depth" or grads != "loss") else _vec(D)   # (g_depth is not passed with g_loss alone)
        g = _backward(c, d, shape, count, grads, want)
        assert g.shape == c["logp"].shape and g.dtype == torch.float32
        rec.note(want, form, "g:" + grads, g, r["g_logp"], U.bound(r, want)["g_logp"], case)
        out[grads] = (g, r)
    if consistency:
        assert _bits(depth).equal(_bits(ops.dpv_expect(d["logp"], d["dc"], BV_log=True))), case
        l2, c2, d2 = _forward(c, d, shape, fwd_expect)
        assert _bits(l2).equal(_bits(loss)) and _bits(c2).equal(_bits(count)) and _bits(d2).equal(_bits(depth)), case
        assert _bits(_backward(c, d, shape, count, "both", expect)).equal(_bits(out["both"][0])), case
    return out


@pytest.mark.parametrize("D", U.PROBE_D)
def test_backward_on_the_vec4_kernels(dev, D):
    rec = _Worst()
    kinds = ("values", "values", "zero_item", "none")
    for i, hw in enumerate(U.PROBE_HW):
        for j, form in enumerate(FORMS):
            _grad_case(rec, dev, (2, D, *hw), form, 6300 + 4 * D + 2 * i + j, _vec(D), kinds[2 * i + j if D % 2 else 3 - 2 * i - j],
                       consistency=True)
    assert rec.reached() == {(_vec(D), f) for f in FORMS}
    rec.report("backward, D = %d" % D)


def test_backward_on_the_scalar_kernels(dev):
    rec = _Worst()
    n = 0
    for shape in ((2, 5, 7, 9), (2, 64, 1, 257), (2, 129, 8, 8), (2, 130, 8, 8)):
        for form in FORMS:
            _grad_case(rec, dev, shape, form, 6400 + n, U.SCALAR, ("values", "binary")[n % 2], consistency=True)
            n += 1
    for form, offs in (("label", ("logp", "label", "mask", "g_depth")), ("depth", ("logp", "depth_gt", "mask", "g_depth"))):
        for off in offs:
            _grad_case(rec, dev, (2, 64, 9, 12), form, 6400 + n, U.SCALAR, "values", off=off)
            n += 1
    assert {(U.SCALAR, f) for f in FORMS} <= rec.reached()
    rec.report("backward, scalar")


# ---- from-depth edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var,pw", U.DEPTH_FORMS, ids=["var%g-pow%g" % vp for vp in U.DEPTH_FORMS])
def test_from_depth_edges(dev, var, pw):
    """Every pixel's ce and every element of g_logp at D = 8 (and 33) for one (variance, pow): the edge placements of
    util_soft_ce.depth_maps (on a candidate, midway, below, above, far out) are pixels 2 .. 6 of every item, badz adds a NaN and a
    +inf.  With no mask and g_loss > 0 an element of g_logp is > 0 exactly under the -1 label (c < 0, label in [0, 1] or -1)."""
    rec = _Worst()
    n = 0
    for D, hw, expect in ((8, (13, 20), "vec8"), (8, (7, 9), U.SCALAR), (33, (9, 12), "vec16")):
        r, c = _probe(rec, dev, D, hw, "depth", 6500 + n, expect, var, pw)
        dc, flat = c["dc"], c["depth_gt"].flatten()   # (none of the placements was in the band and drawn again)
        assert flat[2] == dc[D // 2] and dc[D // 2] < flat[3] < dc[D // 2 + 1] and flat[4:7].tolist() == [3.0, 45.0, 60.0]
        if var == 0.01 and D == 8:
            z, minus = c["depth_gt"], r["minus"]
            assert int((minus & (z > 5) & (z < 40)).sum()) > 5 and int((~minus).sum()) > 5   # -1 pixels inside the range
        for family in ("soft2", "badz"):
            out = _grad_case(rec, dev, (2, D, *hw), "depth", 6550 + n, expect, "none", var, pw, family=family)
            g, r2 = out["loss"]
            minus_gpu = (g > 0).all(1).cpu()
            assert torch.equal(minus_gpu, r2["minus"]) and torch.equal((g > 0).any(1).cpu(), r2["minus"]), (D, hw, family)
            if family == "badz":
                assert bool(r2["minus"].view(2, -1)[0, 7]) and bool(r2["minus"].view(2, -1)[1, 9])
            n += 1
    assert {p for p, _ in rec.reached()} == {"vec8", "vec16", U.SCALAR}
    rec.report("from depth, variance %g pow %g" % (var, pw))


# ---- non-finite logp --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", U.NONFINITE)
def test_nonfinite_logp_by_class(dev, family):
    rec = _Worst()
    n = 0
    for shape, expect in (((3, 16, 9, 12), "vec8"), ((3, 100, 13, 20), "vec32"), ((3, 16, 7, 9), U.SCALAR)):
        for form in FORMS:
            out = _grad_case(rec, dev, shape, form, 6600 + n, expect, "binary", family=family)
            r = out["both"][1]
            assert bool((r["ce"][0] == float("inf")).any()) and bool(torch.isfinite(r["g_logp"]).all())
            if family == "nonfinite":
                assert float(r["loss"][0]) == float("inf") and bool(r["loss"][1].isnan()) == (form == "label")
            else:
                assert bool(torch.isfinite(r["loss"]).all())
            # every pixel of item 0 (the +inf) and, with a label tensor, of item 1 (the NaN) through probes
            H, W = shape[2:]
            c = U.make_case(family, form, shape, 6600 + n, "binary")
            for item in (0, 1):
                one = {k: (v[item:item + 1].clone() if torch.is_tensor(v) and k != "dc" else v) for k, v in c.items()}
                one["mask"] = None
                r1 = U.case_reference(one, grads=None)
                one["mask"] = torch.eye(H * W).view(H * W, H, W)
                d = _to_dev(one, dev, repeat=H * W)
                loss, count, _ = _forward(one, d, (H * W, shape[1], H, W), expect, want_depth=False)
                E = U.probe_bound(r1, U.bound(r1, expect)["ce"], expect)
                rec.note(expect, form, "ce", loss.view(1, H, W), r1["ce"], E, "%s item %d probes" % (family, item))
                assert int((~torch.isfinite(r1["ce"])).sum()) == (0 if (item == 1 and form == "depth") else 1)
            n += 1
    rec.report("non-finite logp, %s" % family)
