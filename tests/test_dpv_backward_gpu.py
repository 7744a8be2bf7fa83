"""The backward of the DPV reductions (csrc/dpv_bwd.hip) against the float64 references of tests/util_dpv_backward.py, element by
element within the a-priori bound derived there, on every shape of its case table, every column kind and every subset of the
incoming gradients; then the wiring of the autograd Functions of ops around it, bit for bit (the kernel has no atomics).

The kernel is fed a logp the test makes itself (the float64 log-softmax rounded to float32), so the forward kernels cannot
loosen the bound; test_dpv_backward_host.py shows float32 evaluations of the right formula inside the bound (the restatement
of the kernel's loops: 0.74 ... 0.96 of it) and five planted mistakes at least 9.5e3 times outside.

Measured on an MI355X (printed by the tests, -s), worst err / bound per case over all kinds and subsets, dpv_reduce_backward /
dpv_expect_backward with BV_log (the host's figures for the restatement / torch float32 in brackets):
  1x1x1x1 0.00 / 0.24 (0.00 / 0.24), 1x2x1x3 0.74 / 0.20 (0.74 / 0.20), 2x3x4x4 0.84 / 0.48 (0.84 / 0.48),
  3x31x16x16 0.96 / 0.66 (0.96 / 0.65), 2x32x1x257 0.94 / 0.63 (0.94 / 0.63), 2x33x8x36 0.93 / 0.69 (0.93 / 0.62),
  1x64x16x24 0.96 / 0.64 (0.96 / 0.64), 2x65x12x20 0.92 / 0.67 (0.92 / 0.60), 1x128x4x68 0.96 / 0.62 (0.96 / 0.60),
  2x129x4x8 0.95 / 0.62 (0.95 / 0.62), 1x200x3x5 0.90 / 0.60 (0.90 / 0.63).
  The kernel sits where the restatement of its loops sits: the bound is tight (two additions rounding by u |g_logp| each
  against 2 u |g_logp|), and the kernel does what was counted.
With d_{k+1} planted for d_k in a scratch copy of the kernel, test_reduce_backward_against_float64 fails on every case with
D >= 2 (6 ... 24576 elements, up to 9.9e5 times the bound) and test_non_finite_inputs_stay_in_their_pixel fails with it.
"""
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from util import to_dev
import util_dpv_backward as U
import util_dpv_forward as UF

pytestmark = pytest.mark.gpu

IDX = list(range(len(U.CASES)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _on(gs, dev):
    return tuple(None if g is None else g.to(dev) for g in gs)


# ---- the kernels against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_reduce_backward_against_float64(dev, idx):
    c, D = U.case(idx), U.CASES[idx][1]
    dc = c["dc"].to(dev)
    worst = (0.0, None)
    for kind in U.kinds_for(D):
        for sub in U.SUBSETS:
            r = U.reference(idx, kind, sub)
            gl, gp, gd = _on(U.grads_of(c, sub), dev)
            got = _native.dpv_reduce_backward(r["lp32"].to(dev), dc, g_logp=gl, g_prob=gp, g_depth=gd).cpu()
            assert got.shape == r["g64"].shape and got.dtype == torch.float32
            w = U.ratio(got, r["g64"], r["bound"])
            if float(w.max()) > worst[0]:
                worst = (float(w.max()), (kind, sub))
            assert bool((w <= 1.0).all()), "%s %s %s: %d elements beyond the bound, worst %.3g times" % (
                U.CASE_IDS[idx], kind, sub, int((w > 1.0).sum()), float(w.max()))
    print("%s: dpv_reduce_backward worst err / bound = %.2f %s" % (U.CASE_IDS[idx], worst[0], worst[1]))


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_expect_backward_against_float64(dev, idx):
    c, e = U.case(idx), U.expect_reference(idx)
    dpv, dc, gd = e["dpv"].to(dev), c["dc"].to(dev), c["g_depth"].to(dev)
    got = _native.dpv_expect_backward(dpv, dc, True, gd).cpu()
    w = U.ratio(got, e["g64"], e["bound"])
    print("%s: dpv_expect_backward BV_log worst err / bound = %.2f" % (U.CASE_IDS[idx], float(w.max())))
    assert bool((w <= 1.0).all()), (U.CASE_IDS[idx], float(w.max()))
    assert torch.equal(_native.dpv_expect_backward(dpv, dc, False, gd).cpu(), e["plain32"])


def test_non_finite_inputs_stay_in_their_pixel(dev):
    """One pixel with a NaN logit, one with an all -inf column: those two columns of the gradient are non-finite (and equal
    torch float32 autograd on the CPU wherever that is finite); every other element is within the bound."""
    idx = U.NONFINITE_CASE
    c, x = U.case(idx), U.nonfinite_logits()
    lp = U.logp64(x)
    bad = (~torch.isfinite(lp).all(1, keepdim=True)).expand_as(lp)
    assert int(bad[:, 0].sum()) == 2
    dc = c["dc"].to(dev)
    for sub in U.SUBSETS:
        gs = U.grads_of(c, sub)
        gl, gp, gd = _on(gs, dev)
        got = _native.dpv_reduce_backward(lp.float().to(dev), dc, g_logp=gl, g_prob=gp, g_depth=gd).cpu()
        assert not bool(torch.isfinite(got[bad]).any()), sub
        t32 = U.autograd(x, c["dc"], *gs, dtype=torch.float32)
        fin = bad & torch.isfinite(t32)
        assert torch.equal(got[fin], t32[fin]), sub
        w = U.ratio(got, U.closed_form64(lp, c["dc"], *gs), U.reduce_bound(lp, c["dc"], *gs))
        assert bool((w[~bad] <= 1.0).all()), (sub, float(w[~bad].max()))
    e = _native.dpv_expect_backward(lp.float().to(dev), dc, True, c["g_depth"].to(dev)).cpu()
    g64, bound = U.expect_g64_and_bound(lp.float(), c["dc"], c["g_depth"])
    assert not bool(torch.isfinite(e[bad]).any())
    assert bool((U.ratio(e, g64, bound)[~bad] <= 1.0).all())


# ---- the wiring, bit for bit -----------------------------------------------------------------------------------------------
def _check_forward(logp, idx, op, a0=None):
    """The forward's logp against the float64 log-softmax of the float32 input (logits + addend formed in float32): every element
    inside the per-element bound of tests/util_dpv_forward.py, in the summation order the dispatch gives `op` on this shape."""
    r = UF.reference(idx, "randn3", a0 is not None)
    if a0 is not None:
        assert torch.equal(a0.cpu(), UF.addend(idx))
    E = UF.bound(idx, "randn3", a0 is not None, UF.order_of(op, U.CASES[idx]))
    w = UF.worst(logp, r["f"]["logp"], E["logp"])
    assert w <= 1.0, (U.CASE_IDS[idx], op, w)


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_reduce_wiring_is_the_native_call(dev, idx):
    c = U.case(idx)
    B, D, H, W = U.CASES[idx]
    x0, dc = U.logits(idx, "randn3").to(dev), c["dc"].to(dev)
    g = dict(zip(("logp", "prob", "depth"), _on(U.grads_of(c, U.ALL3), dev)))
    bwd = lambda logp, **kw: _native.dpv_reduce_backward(logp.detach(), dc, **kw)
    # every subset of the outputs used in the loss: an unused output arrives as None
    for used in U.SUBSETS:
        names = [k for k, on in zip(("logp", "prob", "depth"), used) if on]
        x = x0.clone().requires_grad_(True)
        r = ops.dpv_reduce_ex(x, dc, want_logp=True, want_prob=True, want_depth=True, inplace=True)
        sum((r[k] * g[k]).sum() for k in names).backward()
        assert torch.equal(x.grad, bwd(r["logp"], **{"g_" + k: g[k] for k in names})), used
        assert torch.equal(x.detach(), x0)   # inplace under autograd leaves the input untouched
        _check_forward(r["logp"], idx, "reduce_ex")
    for used in ((True, False), (False, True), (True, True)):
        names = [k for k, on in zip(("logp", "depth"), used) if on]
        x = x0.clone().requires_grad_(True)
        logp, depth = ops.dpv_reduce(x, dc, want_logp=True, want_depth=True, inplace=True)
        sum(({"logp": logp, "depth": depth}[k] * g[k]).sum() for k in names).backward()
        assert torch.equal(x.grad, bwd(logp, **{"g_" + k: g[k] for k in names})), used
        assert torch.equal(x.detach(), x0)
        _check_forward(logp, idx, "reduce")
    # want_logp=False with the depth used: the Function keeps the logp it does not return
    x = x0.clone().requires_grad_(True)
    none, depth = ops.dpv_reduce(x, dc, want_logp=False, want_depth=True)
    assert none is None
    (depth * g["depth"]).sum().backward()
    with torch.no_grad():
        logp = ops.dpv_reduce(x0, dc, want_logp=True, want_depth=True)[0]
    assert torch.equal(x.grad, bwd(logp, g_depth=g["depth"]))
    r = ops.dpv_reduce_ex(x0.clone().requires_grad_(True), dc, want_logp=False, want_depth=True)
    assert sorted(r) == ["depth"]
    # expanded and strided incoming gradients
    x = x0.clone().requires_grad_(True)
    logp, depth = ops.dpv_reduce(x, dc)
    depth.sum().backward()
    assert torch.equal(x.grad, bwd(logp, g_depth=torch.ones(B, H, W, device=dev)))
    x = x0.clone().requires_grad_(True)
    logp, _ = ops.dpv_reduce(x, dc)
    logp.mean().backward()
    each = (torch.ones((), device=dev) / logp.numel()).expand(B, D, H, W).contiguous()
    assert torch.equal(x.grad, bwd(logp, g_logp=each))
    x = x0.clone().requires_grad_(True)
    logp, _ = ops.dpv_reduce(x, dc)
    w = g["logp"].permute(0, 2, 3, 1).contiguous()
    (logp.permute(0, 2, 3, 1) * w).sum().backward()
    assert torch.equal(x.grad, bwd(logp, g_logp=g["logp"]))


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_addend_wiring(dev, idx):
    """Only the logits, only the addend, or both require grad: the gradient is the native call on the returned logp, and with
    both the two gradients are equal bit for bit."""
    c = U.case(idx)
    x0, dc = U.logits(idx, "randn3").to(dev), c["dc"].to(dev)
    a0 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(7400 + idx)).to(dev)
    g = dict(zip(("logp", "prob", "depth"), _on(U.grads_of(c, U.ALL3), dev)))
    for gx, ga in ((True, False), (False, True), (True, True)):
        x, a = x0.clone().requires_grad_(gx), a0.clone().requires_grad_(ga)
        r = ops.dpv_reduce_ex(x, dc, addend=a, want_logp=True, want_prob=True, want_depth=True)
        sum((r[k] * g[k]).sum() for k in g).backward()
        want = _native.dpv_reduce_backward(r["logp"].detach(), dc, g_logp=g["logp"], g_prob=g["prob"], g_depth=g["depth"])
        assert (x.grad is not None) == gx and (a.grad is not None) == ga
        for got in (x.grad, a.grad):
            assert got is None or torch.equal(got, want), (gx, ga)
        _check_forward(r["logp"], idx, "reduce_ex", a0)
        with torch.no_grad():
            assert torch.equal(r["logp"].detach(), ops.dpv_reduce_ex(x0, dc, addend=a0)["logp"])


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_expect_wiring_is_the_native_call(dev, idx):
    c, e = U.case(idx), U.expect_reference(idx)
    dpv0, dc, gd = e["dpv"].to(dev), c["dc"].to(dev), c["g_depth"].to(dev)
    for bv_log in (True, False):
        x = dpv0.clone().requires_grad_(True)
        (ops.dpv_expect(x, dc, BV_log=bv_log) * gd).sum().backward()
        assert torch.equal(x.grad, _native.dpv_expect_backward(dpv0, dc, bv_log, gd))
        x = dpv0.clone().requires_grad_(True)
        ops.dpv_expect(x, dc, BV_log=bv_log).sum().backward()   # an expanded gradient
        assert torch.equal(x.grad, _native.dpv_expect_backward(dpv0, dc, bv_log, torch.ones_like(gd)))


# ---- the fused tail --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wants", [(True, False, False), (False, True, False), (False, False, True), (True, True, True),
                                   (False, True, True), (True, False, True)])
def test_sweep_dpv_tail_is_the_native_calls(dev, wants):
    """ops.sweep_dpv under autograd = _native.sweep_backward on g = dpv_reduce_backward(logp, g_logp, g_depth) + g_cost: g_ref
    bit for bit, g_src (summed with atomics) to the 1e-6 max|g_src| of test_gradients_reproducible."""
    want_cost, want_logp, want_depth = wants
    B, C, D, H, W, V = 2, 8, 16, 16, 32, 1
    d = to_dev(synth.make_batch(28, B, C=C, D=D, H=H, W=W, V=V, pose="mono"), dev)
    gen = torch.Generator().manual_seed(12)
    gc, gl, gd = (torch.randn(B, D, H, W, generator=gen).to(dev), torch.randn(B, D, H, W, generator=gen).to(dev),
                  torch.randn(B, H, W, generator=gen).to(dev))
    cam = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"])
    sigma = 10.0
    ref, src = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
    cost, logp, depth = ops.sweep_dpv(ref, src, *cam, d["d_candi"], sigma, want_cost=want_cost, want_logp=want_logp,
                                      want_depth=want_depth)
    assert (cost is not None, logp is not None, depth is not None) == wants
    sum((o * g).sum() for o, g, on in ((cost, gc, want_cost), (logp, gl, want_logp), (depth, gd, want_depth)) if on).backward()
    dc = ops.d_candi_tensor(d["d_candi"], dev)
    g = None
    if want_logp or want_depth:
        with torch.no_grad():   # the logp this forward kept: the same fused call, with logp returned
            kept = ops.sweep_dpv(d["ref"], d["src"], *cam, d["d_candi"], sigma, want_cost=want_cost, want_logp=True,
                                 want_depth=want_depth)[1]
        if want_logp:
            assert torch.equal(kept, logp.detach())
        g = _native.dpv_reduce_backward(kept, dc, g_logp=gl if want_logp else None, g_depth=gd if want_depth else None)
    if want_cost:
        g = gc if g is None else g + gc
    g_ref, g_src = _native.sweep_backward(d["ref"], d["src"], *cam, dc, g, sigma, _native.METRIC_L2)
    assert torch.equal(ref.grad, g_ref)
    assert float((src.grad - g_src).abs().max()) <= 1e-6 * float(g_src.abs().max())


# ---- double backward -------------------------------------------------------------------------------------------------------
def _second_order_calls(dev):
    B, D, H, W = 2, 16, 16, 32
    gen = torch.Generator().manual_seed(13)
    dc = torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0)).float().to(dev)
    x0 = torch.randn(B, D, H, W, generator=gen).to(dev)
    lp0 = torch.log_softmax(x0, dim=1)
    dmaps = (3 + 39 * torch.rand(B, H, W, generator=gen)).to(dev)
    masks = (torch.rand(B, H, W, generator=gen) < 0.5).float().to(dev)
    d = to_dev(synth.make_batch(29, B, C=8, D=D, H=H, W=W, V=1, pose="mono"), dev)

    def sweep(ref):
        return ops.sweep_cost(ref, d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)

    return {
        "dpv_reduce": (x0, lambda x: ops.dpv_reduce(x, dc)[1]),
        "dpv_reduce_ex": (x0, lambda x: ops.dpv_reduce_ex(x, dc, want_logp=False, want_prob=True)["prob"]),
        "dpv_expect": (lp0, lambda x: ops.dpv_expect(x, dc, BV_log=True)),
        "dpv_fuse": (lp0, lambda x: ops.dpv_fuse(x, dmaps, masks, dc)[0]),
        "dpv_soft_ce": (lp0, lambda x: ops.dpv_soft_ce(x, dc, depth_gt=dmaps, variance=0.3)[0]),
        "sweep_cost": (d["ref"], sweep),
    }


@pytest.mark.parametrize("name", ["dpv_reduce", "dpv_reduce_ex", "dpv_expect", "dpv_fuse", "dpv_soft_ce", "sweep_cost"])
def test_double_backward_is_refused(dev, name):
    """A HIP backward is not differentiable: with create_graph=True its result must not pass for a constant.  The loss is
    quadratic in the output, so the incoming gradient depends on the input and a second-order gradient exists."""
    x0, fn = _second_order_calls(dev)[name]
    x = x0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((fn(x) ** 2).sum(), x, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
