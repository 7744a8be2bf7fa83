"""The correlation operator on every kernel path and LDS regime against the float64 restatement of tests/util_correlation.py:
every element of the forward and of both gradients inside the a-priori bound derived there (gamma_(n+2) A + (n+2) 2^-126; fp16
I/O one output rounding more), non-finite elements by class, on
  matrix pipe<16|32|64>        C in {1 .. 256} x W in {1 .. 129} x H in {1, 3, 9} x seven (radius, stride2): 40 covering combinations
  scalar<1..4>                 reached by C > 256 (257, 260, 264 at 17 x 33) and by max_displacement > 16 (20, 18, 18, 17; 52 with
                               opt-in LDS), C in {1, 7, 8, 9}, an image smaller than the halo included
  fast backward                max_displacement 4, 8 (LDS <= 64 KiB) and 9, 12, 16, 17 (opt-in LDS), C in {3, 8, 19}, three shapes,
                               each of the three gradient requests (both, x1 only, x2 only)
  beyond the tiled kernels     backward at max_displacement 18, 20, 24 and forward at 148: served by the general kernels
  general                      the seven configurations of tests/test_round3_rows.py, fp32 and fp16, forward and both gradients
with B = 2 and five input families (N(0,1); 100 + N(0,1); x2 = +-x1 alternating over c; N(0,1) x 1e-15 and x 1e+15).  Every case
asserts the kernel it reaches through util_correlation.which_kernel, and every test the set of kernels its cases reached.
Impulses (a single 1 in x1, x2 and grad_out at the image corners and on the tile seams, every displacement of the grid, one batch
item per displacement) must give exactly 1/C at exactly one element and exactly 0 elsewhere; one +inf, -inf and NaN planted in
each of x1, x2 and grad_out must give the reference's class at every element on the tiled, the general and the fp16 paths alike;
two calls give identical bits, and a channel-sliced view the bits of its contiguous copy.

test_correlation_host.py shows float32 emulations of the three summation orders inside the bound (forward 0.59, gradients 0.07 of it
at the worst) and seven planted mistakes at least 86 times outside.

Measured on an MI355X (printed by the tests, -s), worst err / bound per kernel path over all cases of this file:
  matrix pipe<16>              out 0.631 (2x3x21x35, radius 4, stride2 2, x 1e+15); C = 10: 0.260
  matrix pipe<32> / <64>       out 0.026 (2x65x9x64) / 0.028 (2x129x3x129)
  scalar<1> .. <4>             out 0.458, 0.379, 0.586, 0.429 at C <= 9;  0.014, 0.066, 0.076, 0.070 at C in {257, 260, 264}
  fast backward                g1 0.052, g2 0.051 (81 and 25 displacements)
  fast backward, opt-in LDS    g1 0.242, g2 0.248 (max_displacement 17: 9 displacements); 0.075 / 0.070 at 9 .. 16
                               (one gradient alone: the figures of both at once, on every path)
  general, fp32                out 0.356, g1 0.151, g2 0.150; backward at max_displacement 18 .. 24: 0.052 / 0.073; forward at 148: 0.210
  general, fp16                out 0.995, g1 0.977, g2 0.987 (the one rounding of the output is nearly all of that bound)
The ratio falls with the number of terms on every path alike: the bound grows like n u A, the error of a sum of n products of
mixed sign like sqrt(n) u A; at C = 1 .. 3 a single product's rounding, u |a b| / 2 against gamma_3 |a b|, is most of it.  The
matrix-pipe kernel sits where the scalar kernels sit at the same C (v_mfma_f32_16x16x4_f32 rounds like a chain of fmas as far as
this bound can see); no ratio is above 1 and no defect was found in the arithmetic of any kernel.  Against the library of the
commit before this suite, 8 of its 35 tests fail: the backward at max_displacement >= 18 raises (hipErrorInvalidValue from the
tiled launcher's LDS check after a forward that worked), and the general kernels, fp32 and fp16, skip the terms that pair a value
with padding, so an inf there gives inf or a finite value where the tiled kernels and the reference give NaN.
"""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native as N
import util_correlation as U

pytestmark = pytest.mark.gpu

CORR_CONFIGS = [(4, 1, 4, 1, 1), (5, 1, 4, 1, 1), (3, 1, 4, 1, 2), (4, 1, 4, 2, 1), (4, 3, 4, 1, 3), (6, 3, 5, 2, 2), (20, 1, 20, 1, 2)]


def fast(r, s2):
    """The fast configuration of a (radius, stride2): kernel 1, stride1 1, pad = max_displacement = radius * stride2."""
    return (r * s2, 1, r * s2, 1, s2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


class _Worst:
    """Worst err / bound per (kernel path, output), with the case that gave it."""

    def __init__(self):
        self.top = {}

    def note(self, path, name, w, case):
        if w > self.top.get((path, name), (-1.0, None))[0]:
            self.top[(path, name)] = (w, case)

    def paths(self):
        return {p for p, _ in self.top}

    def report(self, tag):
        for (path, name), (w, case) in sorted(self.top.items()):
            print("%s: %-28s %-4s worst err / bound = %.3f  %s" % (tag, path, name, w, case))
        over = {k: v for k, v in self.top.items() if not v[0] <= 1.0}
        assert not over, (tag, over)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _first_over(got, ref, E):
    """The worst element of a result that is outside the bound, for the failure message."""
    r = U.ratio(got, ref, E)
    idx = tuple(int(v) for v in np.unravel_index(int(r.argmax()), tuple(r.shape)))
    return "element %s got %r want %r bound %r" % (idx, float(got.detach().cpu().double()[idx]), float(ref[idx]), float(E[idx]))


def _check(rec, got, r, name, shape, cfg, half, path, case):
    w = U.check(got, r, name, shape, cfg, half)
    rec.note(path, name, w, case)
    if not w <= 1.0:
        _, C, H, W = shape
        E = U.bound(r[name], r["A_" + name], U.terms(C, H, W, cfg, name != "out"), half)
        print("OVER THE BOUND %s %s %s: ratio %.3g, %s" % (path, name, case, w, _first_over(got, r[name], E)))


def _run(rec, dev, shape, cfg, family, seed, half=False, backward=False, expect=None, expect_bwd=None, data=None, repeat=False):
    """One case: forward (and the three gradient requests) against the reference, on the path which_kernel names."""
    x1, x2, go = data if data is not None else U.inputs(family, shape, cfg, seed, half)
    case = "%s %s %s%s" % ("x".join(map(str, shape)), cfg, family, " fp16" if half else "")
    path = U.which_kernel(shape, cfg, half)
    assert expect is None or path == expect, (case, path, expect)
    r = U.reference(x1, x2, go if backward else None, cfg)
    d1, d2 = x1.to(dev), x2.to(dev)
    out = N.correlation_forward(d1, d2, *cfg)
    assert out.dtype == x1.dtype and tuple(out.shape) == tuple(r["out"].shape), case
    h = " fp16" if half else ""
    _check(rec, out, r, "out", shape, cfg, half, path + h, case)
    res = {"out": out}
    if repeat:
        assert _same_bits(out, N.correlation_forward(d1, d2, *cfg)), case
    if backward:
        bpath = U.which_kernel(shape, cfg, half, backward=True)
        assert expect_bwd is None or bpath == expect_bwd, (case, bpath, expect_bwd)
        dg = go.to(dev)
        for want1, want2 in ((True, True), (True, False), (False, True)):
            g1, g2 = N.correlation_backward(d1, d2, dg, *cfg, want1=want1, want2=want2)
            assert (g1 is None) == (not want1) and (g2 is None) == (not want2)
            tag = bpath + h + ("" if want1 and want2 else ", x1 only" if want1 else ", x2 only")
            if want1:
                _check(rec, g1, r, "g1", shape, cfg, half, tag, case)
            if want2:
                _check(rec, g2, r, "g2", shape, cfg, half, tag, case)
            if want1 and want2:
                res.update(g1=g1, g2=g2)
                if repeat:
                    h1, h2 = N.correlation_backward(d1, d2, dg, *cfg)
                    assert _same_bits(g1, h1) and _same_bits(g2, h2), case
    return res, r


# ---- matrix-pipe forward -------------------------------------------------------------------------------------------------------
PIPE_C = (1, 3, 4, 5, 16, 17, 64, 65, 128, 129, 256)
PIPE_W = (1, 15, 16, 17, 63, 64, 65, 129)
PIPE_H = (1, 3, 9)
PIPE_RS = ((1, 1), (4, 1), (3, 2), (3, 5), (2, 8), (1, 16), (4, 4))
# 40 combinations: the four lists have pairwise coprime lengths, so stepping through all of them at once pairs every value of one
# with ever different values of the others
PIPE_CASES = [(PIPE_C[i % 11], PIPE_H[i % 3], PIPE_W[i % 8], PIPE_RS[i % 7], U.FAMILIES[i % 5]) for i in range(40)]


def test_matrix_pipe_forward(dev):
    rec = _Worst()
    for i, (C, H, W, (r, s2), family) in enumerate(PIPE_CASES):
        want = U.MFMA[16 if C <= 64 else 32 if C <= 128 else 64]
        _run(rec, dev, (2, C, H, W), fast(r, s2), family, 4000 + i, expect=want, repeat=i < 3)
    assert {c[0] for c in PIPE_CASES} == set(PIPE_C) and {c[2] for c in PIPE_CASES} == set(PIPE_W)
    assert {c[1] for c in PIPE_CASES} == set(PIPE_H) and {c[3] for c in PIPE_CASES} == set(PIPE_RS)
    assert rec.paths() == set(U.MFMA.values())
    rec.report("matrix pipe")


# ---- scalar forward ------------------------------------------------------------------------------------------------------------
def test_scalar_forward_by_channels(dev):
    """C > 256: the chunk-of-8 tail (257 = 32 * 8 + 1, 260, 264 = 33 * 8), two tiles each way, a ragged last tile."""
    rec = _Worst()
    i = 0
    for C in (257, 260, 264):
        for r in (1, 2, 3, 4):
            _run(rec, dev, (2, C, 17, 33), fast(r, 1), U.FAMILIES[i % 5], 4100 + i, expect=U.SCALAR[r], repeat=i == 0)
            i += 1
    assert rec.paths() == set(U.SCALAR.values())
    rec.report("scalar, C > 256")


def test_scalar_forward_by_displacement(dev):
    """max_displacement > 16: 20, 18, 18, 17 at LDS <= 64 KiB and 52 at 68 KiB (opt-in); 5 x 7 has a halo wider than the image."""
    rec = _Worst()
    i = 0
    for (r, s2) in ((4, 5), (3, 6), (2, 9), (1, 17)):
        for C in (1, 7, 8, 9):
            for H, W in ((5, 7), (16, 16), (17, 33)):
                assert U.forward_lds(r * s2) <= U.LDS_OPT_IN
                _run(rec, dev, (2, C, H, W), fast(r, s2), U.FAMILIES[i % 5], 4200 + i, expect=U.SCALAR[r], repeat=i == 0)
                i += 1
    assert U.LDS_OPT_IN < U.forward_lds(52) <= U.LDS_CAP
    for C, (H, W) in ((8, (17, 33)), (9, (5, 7))):
        _run(rec, dev, (2, C, H, W), fast(4, 13), "randn", 4290 + C, expect=U.SCALAR[4], repeat=True)
    assert rec.paths() == set(U.SCALAR.values())
    rec.report("scalar, md > 16")


# ---- fast backward -------------------------------------------------------------------------------------------------------------
BWD_RS = ((4, 1), (4, 2), (3, 3), (4, 3), (4, 4), (1, 17))   # max_displacement 4, 8 | 9, 12, 16, 17


@pytest.mark.parametrize("rs", BWD_RS, ids=["md%d" % (r * s2) for r, s2 in BWD_RS])
def test_fast_backward(dev, rs):
    r, s2 = rs
    md = r * s2
    want = U.FAST_BWD_OPT_IN if md >= 9 else U.FAST_BWD
    assert (U.backward_lds(md) > U.LDS_OPT_IN) == (md >= 9) and U.backward_lds(md) <= U.LDS_CAP
    rec = _Worst()
    i = 0
    for C in (3, 8, 19):
        for H, W in ((16, 16), (21, 35), (5, 7)):
            _run(rec, dev, (2, C, H, W), fast(r, s2), U.FAMILIES[(i + md) % 5], 4300 + 16 * md + i, backward=True, expect_bwd=want, repeat=i == 0)
            i += 1
    assert {p for p in rec.paths() if p.startswith("fast")} == {want, want + ", x1 only", want + ", x2 only"}
    rec.report("fast backward, md = %d" % md)


# ---- beyond the tiled kernels' LDS ---------------------------------------------------------------------------------------------
def test_beyond_the_tiled_kernels_lds(dev):
    """Backward at max_displacement 18, 20, 24 and forward at 148: the tile does not fit 160 KiB, the general kernels serve the call."""
    rec = _Worst()
    for i, (r, s2) in enumerate(((3, 6), (4, 5), (4, 6))):
        assert U.backward_lds(r * s2) > U.LDS_CAP
        _run(rec, dev, (2, 5, 21, 35), fast(r, s2), U.FAMILIES[i], 4400 + i, backward=True, expect=U.SCALAR[r], expect_bwd=U.GENERAL, repeat=i == 0)
    for cfg in ((20, 1, 20, 1, 5), (18, 1, 18, 1, 6)):   # the two configurations whose backward used to raise
        assert U.which_kernel((2, 5, 9, 11), cfg, backward=True) == U.GENERAL
    assert U.forward_lds(148) > U.LDS_CAP
    _run(rec, dev, (2, 5, 9, 11), fast(4, 37), "randn", 4410, backward=True, expect=U.GENERAL, expect_bwd=U.GENERAL, repeat=True)
    rec.report("beyond the LDS")


# ---- general path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
@pytest.mark.parametrize("ci", range(len(CORR_CONFIGS)), ids=["-".join(map(str, c)) for c in CORR_CONFIGS])
def test_general_path(dev, ci, half):
    cfg = CORR_CONFIGS[ci]
    md = cfg[2]
    shape = (2, 10, 21 if md < 10 else 44, 30 if md < 10 else 47)
    fams = U.HALF_FAMILIES if half else U.FAMILIES
    rec = _Worst()
    for n, family in enumerate(dict.fromkeys(("randn", fams[ci % len(fams)], fams[(ci + 2) % len(fams)]))):
        tiled = ci == 0 and not half   # the reference's own configuration: the tiled kernels in fp32
        _run(rec, dev, shape, cfg, family, 4500 + 8 * ci + n, half=half, backward=True,
             expect=U.MFMA[16] if tiled else U.GENERAL, expect_bwd=U.FAST_BWD if tiled else U.GENERAL, repeat=n == 0)
    rec.report("general %s %s" % (cfg, "fp16" if half else "fp32"))


# ---- impulses ------------------------------------------------------------------------------------------------------------------
IMPULSE_HW = (17, 65)
IMPULSE_AT = [(0, 0), (0, 64), (16, 0), (16, 64)] + [(y, x) for y in (15, 16) for x in (15, 16, 63, 64)]
IMPULSE_CASES = (   # cfg, half, forward path, backward path
    (fast(4, 1), False, U.MFMA[16], U.FAST_BWD),
    (fast(3, 5), False, U.MFMA[16], U.FAST_BWD_OPT_IN),
    (fast(4, 5), False, U.SCALAR[4], U.GENERAL),
    ((5, 1, 4, 1, 1), False, U.GENERAL, U.GENERAL),
    (fast(4, 1), True, U.GENERAL, U.GENERAL),
)


@pytest.mark.parametrize("cfg,half,fpath,bpath", IMPULSE_CASES, ids=["%s-%s" % ("-".join(map(str, c[0])), "fp16" if c[1] else "fp32") for c in IMPULSE_CASES])
def test_impulses_are_exact(dev, cfg, half, fpath, bpath):
    """x1 = 1 at (c, y, x), x2 = 1 at (c, y + dy, x + dx), grad_out = 1 at (d, y, x), zero elsewhere: out is 1/C at (d, y, x) alone,
    d x1 is 1/C at (c, y, x) alone, d x2 is 1/C at (c, y + dy, x + dx) alone -- and all three are zero everywhere when the x2 texel is
    outside the image.  Batch item b carries displacement b, so one call covers the grid (and every batch offset)."""
    pad, k, md, s1, s2 = cfg
    assert k == 1 and s1 == 1
    H, W = IMPULSE_HW
    C = 3
    _, dr, ds, oH, oW = U.geometry(H, W, cfg)
    B = ds * ds
    shape = (B, C, H, W)
    assert U.which_kernel(shape, cfg, half) == fpath and U.which_kernel(shape, cfg, half, backward=True) == bpath
    dt = torch.float16 if half else torch.float32
    inv = (torch.tensor(1.0) / torch.tensor(float(C))).to(dt)   # fl32(1 * 1 * fl32(1 / C)), rounded once more for fp16 output
    for n, (y, x) in enumerate(IMPULSE_AT):
        c = n % C
        x1, x2 = torch.zeros(shape, dtype=dt), torch.zeros(shape, dtype=dt)
        go = torch.zeros(B, B, oH, oW, dtype=dt)
        e_out, e1, e2 = torch.zeros_like(go), torch.zeros_like(x1), torch.zeros_like(x2)
        oy, ox = y + pad - md, x + pad - md
        for b in range(B):
            dy, dx = (b // ds - dr) * s2, (b % ds - dr) * s2
            x1[b, c, y, x] = 1
            go[b, b, oy, ox] = 1
            if 0 <= y + dy < H and 0 <= x + dx < W:
                x2[b, c, y + dy, x + dx] = 1
                e_out[b, b, oy, ox] = inv
                e1[b, c, y, x] = inv
                e2[b, c, y + dy, x + dx] = inv
        d1, d2, dg = x1.to(dev), x2.to(dev), go.to(dev)
        out = N.correlation_forward(d1, d2, *cfg)
        g1, g2 = N.correlation_backward(d1, d2, dg, *cfg)
        for name, got, want in (("out", out, e_out), ("g1", g1, e1), ("g2", g2, e2)):
            got = got.cpu()
            assert torch.equal(got, want), (name, (y, x), int((got != want).sum()), (got != want).nonzero()[:4].tolist())
        assert int((e_out != 0).sum()) >= B // 4   # (at a corner a quarter of the grid stays inside the image)


# ---- non-finite inputs ---------------------------------------------------------------------------------------------------------
NONFINITE = (   # cfg, shape, forward path, backward path
    (fast(4, 1), (2, 5, 17, 33), U.MFMA[16], U.FAST_BWD),
    (fast(4, 3), (2, 5, 17, 33), U.MFMA[16], U.FAST_BWD_OPT_IN),
    (fast(4, 5), (2, 5, 17, 33), U.SCALAR[4], U.GENERAL),
    (fast(4, 37), (2, 5, 9, 33), U.GENERAL, U.GENERAL),
    ((6, 3, 5, 2, 2), (2, 5, 17, 33), U.GENERAL, U.GENERAL),
)


@pytest.mark.parametrize("cfg,shape,fpath,bpath", NONFINITE, ids=["-".join(map(str, c[0])) for c in NONFINITE])
def test_nonfinite_classes_agree_on_every_path(dev, cfg, shape, fpath, bpath):
    """One +inf, one -inf and one NaN in each of x1, x2 and grad_out (a corner, beside the tile seam, the interior): every output
    element has the reference's class and the finite ones are inside the bound -- through the fp32 entry (tiled kernels where the
    configuration has them), through the fp16 entry (general kernels) and, for a fast configuration, through the general fp32
    kernels with pad one larger, whose output is the same inside a ring of one more pixel."""
    rec = _Worst()
    data = U.plant_nonfinite(*U.inputs("randn", shape, cfg, 4600 + cfg[0]))
    res32, r32 = _run(rec, dev, shape, cfg, "nonfinite", 0, backward=True, expect=fpath, expect_bwd=bpath, data=data, repeat=True)
    data16 = tuple(t.half() for t in data)
    res16, r16 = _run(rec, dev, shape, cfg, "nonfinite", 0, half=True, backward=True, expect=U.GENERAL, expect_bwd=U.GENERAL, data=data16)
    rec.report("non-finite %s" % (cfg,))
    for name in ("out", "g1", "g2"):
        c32, c16 = U.classes(res32[name].cpu()), U.classes(res16[name].cpu())
        assert torch.equal(c32, c16), name
        assert torch.equal(c32, U.classes(r32[name])) and int((c32 != 0).sum()) > 0, name
    assert int((U.classes(r32["out"]) == 3).sum()) > 0   # an inf met the padding
    if U.fast_path(cfg):
        pad, k, md, s1, s2 = cfg
        wide = (pad + 1, k, md, s1, s2)
        assert U.which_kernel(shape, wide) == U.GENERAL
        out = N.correlation_forward(data[0].to(dev), data[1].to(dev), *wide)
        rw = U.reference(data[0], data[1], None, wide)
        rec2 = _Worst()
        _check(rec2, out, rw, "out", shape, wide, False, U.GENERAL, "pad + 1")
        rec2.report("non-finite, pad + 1")
        assert torch.equal(U.classes(out.cpu()[:, :, 1:-1, 1:-1]), U.classes(res32["out"].cpu()))


# ---- views -----------------------------------------------------------------------------------------------------------------------
def test_a_channel_sliced_view_gives_the_bits_of_its_copy(dev):
    for cfg, half in ((fast(4, 1), False), (fast(4, 5), False), ((5, 1, 4, 1, 1), False), (fast(4, 1), True)):
        x1, x2, go = (t.to(dev) for t in U.inputs("randn", (2, 12, 17, 33), cfg, 4700, half))
        v1, v2 = x1[:, 1:11:2], x2[:, 2:12:2]
        assert not v1.is_contiguous() and not v2.is_contiguous()
        c1, c2 = v1.contiguous(), v2.contiguous()
        assert _same_bits(N.correlation_forward(v1, v2, *cfg), N.correlation_forward(c1, c2, *cfg))
        gv = go.transpose(2, 3).contiguous().transpose(2, 3)   # the same values, another memory order
        assert not gv.is_contiguous() and torch.equal(gv, go)
        for a, b in zip(N.correlation_backward(v1, v2, gv, *cfg), N.correlation_backward(c1, c2, go, *cfg)):
            assert _same_bits(a, b)
