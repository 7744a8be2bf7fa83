"""GPU suite: ops.dpv_fuse, forward (csrc/dpv_fuse.hip: dpv_fuse_reg_kernel<64|128>, dpv_fuse_kernel) and backward
(csrc/dpv_fuse_bwd.hip: the register form FULL and !FULL, the re-reading form with the fast and with libm's arithmetic), against
the float64 restatement of tests/util_fuse.py inside its a-priori bound on every plane of every column -- no pixel is left
out -- and the two claims no reference can check: that the backward recomputes the forward's q bit for bit, and that it
decides the clamp on the number the forward clamped.  test_fuse_host.py shows a float32 evaluation inside the same bound and
six wrong kernels outside it through the same comparison functions.

  case          forward      backward       exercises
  3x1x1x1       reg<64>      !FULL          one plane, one pixel; B = 3
  2x2x1x255     reg<64>      !FULL          two planes, a workgroup one pixel short
  3x63x9x37     reg<64>      !FULL          one plane short of FULL, 333 pixels, B = 3
  3x64x16x16    reg<64>      FULL           exactly one workgroup, B = 3
  1x64x257x1    reg<64>      FULL           one live lane in the second workgroup, W = 1
  3x65x257x1    reg<128>     general-fast   the first D the backward re-reads; B = 3
  1x128x16x16   reg<128>     general-fast   the last D of the fast arithmetic
  3x129x1x255   libm         general-libm   the first D of libm's; B = 3, H = 1
  1x200x9x37    libm         general-libm   D well past
Every case holds the column kinds of util_fuse.KINDS on its first pixels.

Measured on an MI355X (printed by the tests, -s), worst error / bound:
  forward, fused / log fused: 3x1x1x1 0 / 0, 2x2x1x255 0.284 / 0.317, 3x63x9x37 0.211 / 0.280, 3x64x16x16 0.203 / 0.270,
    1x64x257x1 0.215 / 0.272, 3x65x257x1 0.205 / 0.289, 1x128x16x16 0.154 / 0.231, 3x129x1x255 0.175 / 0.208,
    1x200x9x37 0.130 / 0.208.
  backward, g_f / g_l / both: 3x1x1x1 0 / 0 / 0, 2x2x1x255 0.247 / 0.742 / 0.583, 3x63x9x37 0.171 / 0.979 / 0.910,
    3x64x16x16 0.175 / 0.989 / 0.895, 1x64x257x1 0.178 / 0.971 / 0.867, 3x65x257x1 0.227 / 0.957 / 0.907,
    1x128x16x16 0.131 / 0.954 / 0.845, 3x129x1x255 0.134 / 0.970 / 0.970, 1x200x9x37 0.412 / 0.956 / 0.941.  With g_l the
    gradient is g_l - q T and the bound hardly more than that subtraction's rounding u |g_x|; the host emulation gives the same
    figures.
  dead columns against softmax(logp): 0.003 ... 0.009; the same bits on all nine dead columns of a case.
  q of the forward against q of the backward: 0 planes differ of 888 + 45440 + 34880 + 11684 + 36037 + 21853 + 68511 +
    44628 = 263921 compared (D = 1 has no second plane to probe from).
  the clamp: D = 64: 42 of 63 ladder planes cross, 23520 plane-pixels above eps, 0 disagreements; D = 128: 85 of 127, 33872, 0.
  band columns (depth 47.3 ... 47.8): reg<64> / FULL the -1 rule on all six; reg<128> / general-fast the quotient at 47.3 and
    47.4, then the -1 rule; libm the quotient on all six.  Band columns in the value tests: 0.
No defect was found in either kernel.
"""
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops
import util_fuse as U

pytestmark = pytest.mark.gpu

IDX = range(len(U.CASES))
DEAD_IDX = [i for i in IDX if U.CASES[i][0] * U.CASES[i][2] * U.CASES[i][3] >= len(U.KINDS)]   # the cases that hold every kind
EPS32 = torch.tensor(U.EPS, dtype=torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _on(dev, c):
    return tuple(c[k].to(dev) for k in ("logp", "dmaps", "masks", "dc", "g_f", "g_l"))


def _forward(dev, idx):
    """(fused, log fused) of the case on the device, computed once."""
    def make():
        logp, dmaps, masks, dc, _, _ = _on(dev, U.case(idx))
        return ops.dpv_fuse(logp, dmaps, masks, dc, var=U.VAR)
    return U.cached(("gpu_forward", idx), make)


def _autograd(logp, dmaps, masks, dc, g_f, g_l):
    x = logp.detach().clone().requires_grad_(True)
    fused, logf = ops.dpv_fuse(x, dmaps, masks, dc, var=U.VAR)
    total = 0
    if g_f is not None:
        total = total + (fused * g_f).sum()
    if g_l is not None:
        total = total + (logf * g_l).sum()
    total.backward()
    return x.grad


def _backward(logp, dmaps, masks, dc, g_f=None, g_l=None):
    return _native.dpv_fuse_backward(logp, dmaps, masks, dc, U.VAR, U.EPS, g_fused=g_f, g_logfused=g_l)


def _c_entry(logp, dmaps, masks, dc):
    """pdepth_dpv_fuse_f32 called directly, on the null stream."""
    B, D, H, W = logp.shape
    cf, cl = torch.full_like(logp, -7.0), torch.full_like(logp, -7.0)
    torch.cuda.synchronize()
    rc = _native.load().pdepth_dpv_fuse_f32(logp.data_ptr(), dmaps.data_ptr(), masks.data_ptr(), dc.data_ptr(), B, D, H, W,
                                            U.VAR, U.EPS, cf.data_ptr(), cl.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _native.load().pdepth_last_error().decode()
    return cf, cl


# ---- values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_forward_inside_the_bound_on_every_plane(dev, idx):
    logp, dmaps, masks, dc, _, _ = _on(dev, U.case(idx))
    fused, logf = _forward(dev, idx)
    rf, rl = U.check_forward(idx, fused, logf)
    print("%s forward: fused %.3f, log fused %.3f of the bound, band columns %d" % (U.CASE_IDS[idx], rf, rl, U.reference(idx)["n_band"]))
    assert rf <= 1 and rl <= 1
    # masks in the reference's layout [B,1,H,W]; the partial requests; the C entry called directly: the same bits
    f4, l4 = ops.dpv_fuse(logp, dmaps, masks.unsqueeze(1), dc, var=U.VAR)
    assert torch.equal(f4, fused) and torch.equal(l4, logf)
    only_l = ops.dpv_fuse(logp, dmaps, masks, dc, var=U.VAR, want_fused=False)
    only_f = ops.dpv_fuse(logp, dmaps, masks, dc, var=U.VAR, want_log=False)
    assert only_l[0] is None and only_f[1] is None
    assert torch.equal(only_l[1], logf) and torch.equal(only_f[0], fused)
    cf, cl = _c_entry(logp, dmaps, masks, dc)
    assert torch.equal(cf, fused) and torch.equal(cl, logf)


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_backward_inside_the_bound_on_every_element(dev, idx, mode):
    c = U.case(idx)
    logp, dmaps, masks, dc, _, _ = _on(dev, c)
    g_f, g_l = (None if g is None else g.to(dev) for g in U.grads_of(c, mode))
    fused, _ = _forward(dev, idx)
    direct = _backward(logp, dmaps, masks, dc, g_f, g_l)
    through = _autograd(logp, dmaps, masks, dc, g_f, g_l)
    assert torch.equal(torch.nan_to_num(direct, nan=-7.0), torch.nan_to_num(through, nan=-7.0))
    r = U.check_backward(idx, mode, direct, fused)
    print("%s backward %s: %.3f of the bound, band columns %d" % (U.CASE_IDS[idx], mode, r, U.reference(idx)["n_band"]))
    assert r <= 1


@pytest.mark.parametrize("idx", DEAD_IDX, ids=[U.CASE_IDS[i] for i in DEAD_IDX])
def test_dead_columns(dev, idx):
    """Every Gaussian is 0, t = -1, the prior eps on every plane whatever the mask: fused is softmax(logp) clamped -- what a
    call with a prior of eps on every plane gives -- inside the bound, the same bits on the three dead kinds (they share their
    log-DPV), and the gradient is finite."""
    c, r = U.case(idx), U.reference(idx)
    fused, logf = (t.cpu() for t in _forward(dev, idx))
    logp, dmaps, masks, dc, g_f, g_l = _on(dev, c)
    grad = _backward(logp, dmaps, masks, dc, g_f, g_l).cpu()
    pixels = [(k, p) for k in U.DEAD_KINDS for p in c["kinds"][k]]
    assert pixels
    f = r["f"]
    worst, first = 0.0, None
    for kind, (b, y, x) in pixels:
        assert bool(f["dead"][b, 0, y, x])
        soft = torch.softmax(c["logp"][b, :, y, x].double(), 0).clamp(U.EPS, 1.0)
        assert float((soft - f["fused"][b, :, y, x]).abs().max()) <= 1e-15
        worst = max(worst, float(U.ratio(fused[b, :, y, x], soft, r["E"]["fused"][b, :, y, x]).max()))
        assert bool(torch.isfinite(grad[b, :, y, x]).all())
        if first is None:
            first = (fused[b, :, y, x], logf[b, :, y, x])
        assert torch.equal(fused[b, :, y, x], first[0]) and torch.equal(logf[b, :, y, x], first[1]), kind
    print("%s: %d dead columns, fused %.3f of the bound against softmax(logp)" % (U.CASE_IDS[idx], len(pixels), worst))
    assert worst <= 1


# ---- the forward and the backward agree ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_forward_and_backward_agree_on_q(dev, idx):
    """g_f absent, g_l one-hot on a passing plane j: c_k = [k = j], T = 1 exactly, and the backward returns -q_k * 1 = -q_k on
    every other plane.  So fused_k == -g_x,k bit for bit wherever fused_k > eps.  Two probes, on the largest and the
    second-largest plane, read every plane once."""
    logp, dmaps, masks, dc, _, _ = _on(dev, U.case(idx))
    fused, _ = _forward(dev, idx)
    p1, p2, _, _ = U.one_hot_probes(fused)
    gx1 = _backward(logp, dmaps, masks, dc, g_l=p1)
    gx2 = _backward(logp, dmaps, masks, dc, g_l=p2)
    differ, compared = U.q_disagreements(fused.cpu(), gx1.cpu(), gx2.cpu())
    above = int((fused > U.EPS).sum())
    print("%s: q of the forward and of the backward differ on %d of %d planes compared (%d planes above eps)"
          % (U.CASE_IDS[idx], differ, compared, above))
    B, D, H, W = logp.shape
    assert compared >= above - B * H * W   # (a column with one plane above eps has no second probe for it)
    assert compared > 0 or D == 1
    assert differ == 0


@pytest.mark.parametrize("D", [64, 128])
def test_forward_and_backward_agree_on_the_clamp(dev, D):
    """near_clamp_ladder: with g_l all ones g_x,k = pass_k - q_k T and q_k T <= 200 * 2^-52, so round(g_x,k) is the backward's
    pass_k.  On every ladder plane: fused_k > eps => pass_k = 1, pass_k = 0 => fused_k == eps."""
    lad = U.ladder(D)
    logp, dmaps, masks, dc = (lad[k].to(dev) for k in ("logp", "dmaps", "masks", "dc"))
    fused, _ = ops.dpv_fuse(logp, dmaps, masks, dc, var=U.VAR)
    gx = _backward(logp, dmaps, masks, dc, g_l=torch.ones_like(logp))
    fused, gx = fused.cpu()[0, 1:].reshape(D - 1, -1), gx.cpu()[0, 1:].reshape(D - 1, -1)
    passk = torch.round(gx)
    assert bool(((passk == 0) | (passk == 1)).all()) and float((gx - passk).abs().max()) <= 200 * 2.0 ** -52
    above = fused > EPS32
    crossing = int((above.any(1) & ~above.all(1)).sum())
    wrong = int((above & (passk == 0)).sum()) + int(((passk == 0) & (fused != EPS32)).sum())
    print("ladder D = %d: %d of %d planes cross the clamp, %d planes above eps, %d at eps with pass, %d disagreements"
          % (D, crossing, D - 1, int(above.sum()), int((~above & (passk == 1)).sum()), wrong))
    assert crossing >= (D - 1) // 3
    assert wrong == 0


# ---- where the value is not pinned -----------------------------------------------------------------------------------------
BAND_DEPTHS = (47.3, 47.4, 47.5, 47.6, 47.7, 47.8)


@pytest.mark.parametrize("D,mode", [(64, "reg<64> / FULL"), (128, "reg<128> / general-fast"), (129, "libm / general-libm")])
def test_band_columns(dev, D, mode):
    """Depths 47.3 ... 47.8 beyond powerf(5, 40, 64, 1): the float32 Gaussian sum is a few denormals or 0, and the reference's
    quotient (the prior on the last candidates) and the -1 rule (softmax(logp)) are both legitimate.  Whichever a kernel takes,
    the outputs are finite and in [eps, 1], sum to 1 within 1e-4 + D eps, and the backward is finite.  D = 64 is the model's
    depth count; 128 and 129 (the same 64 candidates, then 40 + 1e-3 k) show the other two dispatch pairs for DESIGN.md."""
    n = len(BAND_DEPTHS)
    g = torch.Generator().manual_seed(77)
    logp = torch.log_softmax(torch.randn(1, D, 1, n, generator=g), dim=1)
    dc = torch.cat([U.candidates(64), 40.0 + 1e-3 * torch.arange(1, D - 63)])[:D]
    dmaps = torch.tensor(BAND_DEPTHS).view(1, 1, n)
    assert bool(U.classify(dmaps, dc)[2].all())
    masks = torch.ones(1, 1, n)
    a = tuple(t.to(dev) for t in (logp, dmaps, masks, dc))
    fused, logf = ops.dpv_fuse(*a, var=U.VAR)
    grad = _backward(*a, g_f=torch.randn(1, D, 1, n, generator=g).to(dev), g_l=torch.randn(1, D, 1, n, generator=g).to(dev))
    fused, logf, grad = fused.cpu(), logf.cpu(), grad.cpu()
    assert bool(torch.isfinite(fused).all()) and bool(torch.isfinite(logf).all()) and bool(torch.isfinite(grad).all())
    assert bool((fused >= EPS32).all()) and bool((fused <= 1).all())
    assert float((fused.double().sum(1) - 1).abs().max()) <= 1e-4 + D * U.EPS
    soft = torch.softmax(logp.double(), 1)
    took = []
    for i in range(n):
        rule = float((fused[0, :, 0, i].double() - soft[0, :, 0, i]).abs().max()) <= 1e-5
        took.append("-1 rule" if rule else "quotient")
    print("band, %s: %s" % (mode, ", ".join("%.1f %s" % (d, t) for d, t in zip(BAND_DEPTHS, took))))


@pytest.mark.parametrize("idx", [2, 3, 6, 7], ids=[U.CASE_IDS[i] for i in (2, 3, 6, 7)])
def test_non_finite_columns(dev, idx):
    """One NaN plane, every plane -inf, x = +120 (exp overflows): fminf / fmaxf turn the NaN quotient into eps, so the forward
    returns eps (and log eps) on every plane of that pixel where the reference returns NaN; the backward returns non-finite
    values there; every other pixel has the clean run's bits."""
    c = U.case(idx)
    B, D, H, W = c["shape"]
    logp, dmaps, masks, dc, g_f, g_l = _on(dev, c)
    n = len(U.KINDS) * U.ROUNDS   # behind the planted kinds
    pix = [((n + i) // (H * W), ((n + i) // W) % H, (n + i) % W) for i in range(3)]
    bad = logp.clone()
    bad[pix[0][0], D // 2, pix[0][1], pix[0][2]] = float("nan")
    bad[pix[1][0], :, pix[1][1], pix[1][2]] = float("-inf")
    bad[pix[2][0], :, pix[2][1], pix[2][2]] = 120.0
    masks = masks.clone()
    for (b, y, x) in pix:
        masks[b, y, x] = 0.0   # the prior 1 / D: exp(120 - log D) overflows at every D here
    clean = ops.dpv_fuse(logp, dmaps, masks, dc, var=U.VAR) + (_backward(logp, dmaps, masks, dc, g_f, g_l),)
    got = ops.dpv_fuse(bad, dmaps, masks, dc, var=U.VAR) + (_backward(bad, dmaps, masks, dc, g_f, g_l),)
    other = torch.ones(B, H, W, dtype=torch.bool, device=dev)
    log_eps = torch.log(EPS32.double()).item()
    for (b, y, x) in pix:
        other[b, y, x] = False
        assert bool((got[0][b, :, y, x] == EPS32.to(dev)).all())
        assert float((got[1][b, :, y, x].double() - log_eps).abs().max()) <= 1e-5
        assert not bool(torch.isfinite(got[2][b, :, y, x]).any())
    o = other.unsqueeze(1).expand_as(logp)
    for a, b_ in zip(got, clean):
        assert torch.equal(a[o], b_[o])
