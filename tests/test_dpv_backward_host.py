"""CPU only: keeps the references of tests/util_dpv_backward.py honest and shows that the bound the GPU suite
(test_dpv_backward_gpu.py) holds csrc/dpv_bwd.hip to discriminates -- float32 evaluations of the right formula are inside it
on every case, column kind and subset of incoming gradients, the planted mistakes are far outside.

Measured (printed by the tests, -s); worst err / bound per case over all kinds and subsets, for the float32 restatement of
the kernel's loops fed the rounded logp / torch float32 autograd against the bound with its own forward's logp error / the
same against the kernel's bound (recorded, not asserted: see util_dpv_backward):
  1x1x1x1 0.00 / 0.00 / 0.00, 1x2x1x3 0.74 / 0.74 / 0.74, 2x3x4x4 0.84 / 0.84 / 0.85, 3x31x16x16 0.96 / 0.96 / 1.55,
  2x32x1x257 0.94 / 0.92 / 1.56, 2x33x8x36 0.93 / 0.93 / 1.49, 1x64x16x24 0.96 / 0.94 / 1.50, 2x65x12x20 0.92 / 0.92 / 1.48,
  1x128x4x68 0.96 / 0.96 / 1.43, 2x129x4x8 0.95 / 0.94 / 1.11, 1x200x3x5 0.90 / 0.87 / 0.99.
  Both come that close where p_k is small and g_x_k ~ g_logp_k lies just above a power of two (1.025, logp = -14.5, 'offset'):
  two additions that round by up to u |g_logp_k| each against the bound's 2 u |g_logp_k|.
  closed form against torch float64 autograd: at most 0.96 of the same formula at 2^-53 (asserted: 2).
  dpv_expect, BV_log: torch float32 is at most 0.65 of the bound.
The smallest factor by which a planted mistake exceeds the bound, over every case with D >= 2, every kind on which a mistake
can show and every mistake: 9.5e3 (no_gprob, 1x2x1x3, peaked); asserted: at least 100.  Per mistake: d_next 2.6e4,
no_psum 7.6e4, gd_neighbour 3.0e4, no_gprob 9.5e3, exp_logits 2.4e6."""
import pytest
import torch

import pdepth_amd  # noqa: F401
import util_dpv_backward as U

IDX = list(range(len(U.CASES)))


def _worst(got, r, bound=None):
    return float(U.ratio(got, r["g64"], r["bound"] if bound is None else bound).max())


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_closed_form_and_float64_autograd_agree(idx):
    """The two float64 references are the same number to float64 rounding: twice the bound's formula at 2^-53, with the
    error of the autograd's own log_softmax in L's place (each of the two is one evaluation of the chain in float64)."""
    c, D = U.case(idx), U.CASES[idx][1]
    worst = 0.0
    for kind in U.kinds_for(D):
        for sub in U.SUBSETS:
            r, gs = U.reference(idx, kind, sub), U.grads_of(c, sub)
            assert r["g64"].dtype == torch.float64 and bool(torch.isfinite(r["g64"]).all())
            b64 = U.reduce_bound(r["lp64"], c["dc"], *gs, unit=U.EPS64, logp_error=U.torch32_logp_error)
            w = _worst(U.autograd(U.logits(idx, kind), c["dc"], *gs), r, b64)
            assert w <= 2.0, (kind, sub, w)
            worst = max(worst, w)
    print("%s: closed form and float64 autograd differ by at most %.2f of the bound at 2^-53" % (U.CASE_IDS[idx], worst))


def test_addend_enters_the_reference_as_a_float64_sum():
    """The reference of a call with an addend is built from the float64 sum of the two float32 tensors."""
    idx = 2
    c, x = U.case(idx), U.logits(idx, "randn3")
    add = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
    lp = U.logp64(x, add)
    assert torch.equal(lp, U.logp64(x.double() + add.double()))
    g = U.closed_form64(lp, c["dc"], *U.grads_of(c, U.ALL3))
    ga = U.autograd(x, c["dc"], *U.grads_of(c, U.ALL3), addend=add)
    b64 = U.reduce_bound(lp, c["dc"], *U.grads_of(c, U.ALL3), unit=U.EPS64, logp_error=U.torch32_logp_error)
    assert float(U.ratio(ga, g, b64).max()) <= 2.0


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_float32_evaluations_stay_within_the_bound(idx):
    """The kernel's two loops restated in float32 and fed the rounded logp meet the bound the kernel is held to; torch float32
    autograd meets it with its own forward's logp error in L's place."""
    c, D = U.case(idx), U.CASES[idx][1]
    w_re = w_t = w_t_kernel = 0.0
    for kind in U.kinds_for(D):
        x = U.logits(idx, kind)
        for sub in U.SUBSETS:
            r, gs = U.reference(idx, kind, sub), U.grads_of(c, sub)
            a = _worst(U.restatement32(r["lp32"], c["dc"], *gs), r)
            t32 = U.autograd(x, c["dc"], *gs, dtype=torch.float32)
            b = _worst(t32, r, U.reduce_bound(r["lp64"], c["dc"], *gs, logp_error=U.torch32_logp_error))
            assert a <= 1.0 and b <= 1.0, (kind, sub, a, b)
            w_re, w_t, w_t_kernel = max(w_re, a), max(w_t, b), max(w_t_kernel, _worst(t32, r))
    print("%s: worst err / bound: restatement %.2f, torch float32 autograd %.2f (%.2f of the kernel's bound)"
          % (U.CASE_IDS[idx], w_re, w_t, w_t_kernel))


def test_planted_mistakes_leave_the_bound():
    """Each mistake, planted into the restatement, exceeds the bound at least 100 times on every case with D >= 2 and every
    kind on which it can show (util_dpv_backward.planted_kinds).  A condition for the suite to be worth having, not a
    tolerance on the kernel."""
    smallest, per_mistake = (float("inf"), None), {}
    for idx, (_, D, _, _) in enumerate(U.CASES):
        if D < 2:
            continue
        for kind in U.planted_kinds(D):
            for m in U.MISTAKES:
                f = U.planted_factor(idx, kind, m)
                assert f >= 100.0, (U.CASE_IDS[idx], kind, m, f)
                per_mistake[m] = min(per_mistake.get(m, float("inf")), f)
                if f < smallest[0]:
                    smallest = (f, (U.CASE_IDS[idx], kind, m))
    print("smallest factor by which a planted mistake exceeds the bound: %.3g %s" % smallest)
    print("per mistake: " + ", ".join("%s %.3g" % kv for kv in per_mistake.items()))
    # the one combination left out has nothing to catch
    idx = U.CASE_IDS.index("1x2x1x3")
    assert U.planted_kinds(2) == tuple(k for k in U.kinds_for(2) if k != "masked")
    assert all(U.planted_factor(idx, "masked", m) <= 1.0 for m in ("d_next", "gd_neighbour", "no_gprob"))


def test_the_restatement_without_a_mistake_is_the_formula():
    """On a column small enough to do by hand: D = 2, logp = log(1/4, 3/4), d = (2, 6), g_logp = (1, -1), g_prob = (0.5, 0.25),
    g_depth = 2: t = (4.5, 12.25), G = (2.125, 8.1875), S = 10.3125, g_x = (-0.453125, 0.453125)."""
    lp = torch.log(torch.tensor([0.25, 0.75], dtype=torch.float64)).reshape(1, 2, 1, 1)
    dc = torch.tensor([2.0, 6.0])
    gl, gp, gd = torch.tensor([1.0, -1.0]).reshape(1, 2, 1, 1), torch.tensor([0.5, 0.25]).reshape(1, 2, 1, 1), torch.full((1, 1, 1), 2.0)
    want = torch.tensor([-0.453125, 0.453125], dtype=torch.float64).reshape(1, 2, 1, 1)
    assert float((U.closed_form64(lp, dc, gl, gp, gd) - want).abs().max()) <= 1e-15
    got = U.restatement32(lp.float(), dc, gl, gp, gd)
    assert bool(((got.double() - want).abs() <= U.reduce_bound(lp, dc, gl, gp, gd)).all())
    # the gradient of a softmax chain sums to zero over the planes
    r = U.reference(6, "randn3", U.ALL3)
    assert float(r["g64"].sum(1).abs().max()) <= 1e-12 * float(r["g64"].abs().max()) * 64


def test_cases_and_kinds_reach_what_they_are_named_for():
    hw = [h * w for (_, _, h, w) in U.CASES]
    assert 256 in hw and 257 in hw and min(hw) == 1 and any(n % 4 for n in hw)
    assert {d for (_, d, _, _) in U.CASES} >= {1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 200} and max(b for (b, _, _, _) in U.CASES) == 3
    assert len(U.SUBSETS) == 7 and len(set(U.SUBSETS)) == 7
    for idx, (B, D, H, W) in enumerate(U.CASES):
        dc = U.case(idx)["dc"]
        assert dc.dtype == torch.float32 and dc.shape == (D,) and float(dc.min()) >= 0.5 and float(dc.max()) <= 60.0
        assert (idx % 2 == 0) == bool((dc[1:] >= dc[:-1]).all()) or D < 3
        for kind in U.kinds_for(D):
            x = U.logits(idx, kind)
            assert x.shape == (B, D, H, W) and x.dtype == torch.float32
            top = x.amax(1, keepdim=True)
            if kind == "peaked":
                assert bool(((x == top).sum(1) == 1).all()) and bool(((x < top - 50).sum(1) == D - 1).all())
                planes = set(x.argmax(1).flatten().tolist())
                assert 0 in planes and (B * H * W == 1 or D - 1 in planes)
            elif kind == "tie":
                assert bool(((x == top).sum(1) == 2).all())
            elif kind == "flat":
                assert bool((x == top).all())
            elif kind == "offset":
                assert float(x.min()) > 9.9e3
            elif kind == "masked":
                assert bool((torch.isinf(x).sum(1) == max(1, D // 3)).all()) and D - max(1, D // 3) >= 1
            else:
                assert bool(torch.isfinite(x).all())
    lp = U.logp64(U.nonfinite_logits())
    bad = ~torch.isfinite(lp).all(1)
    assert int(bad.sum()) == 2 and all(bool(bad[b, y, x]) for (b, y, x) in U.NONFINITE_PIXELS)


@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_expect_backward_references(idx):
    """dpv_expect: torch float32 autograd is inside the BV_log bound, and without BV_log it is the float32 product."""
    c, e = U.case(idx), U.expect_reference(idx)
    d = c["dc"].view(1, -1, 1, 1)
    for bv_log in (True, False):
        x = e["dpv"].clone().requires_grad_(True)
        (((torch.exp(x) if bv_log else x) * d).sum(1) * c["g_depth"]).sum().backward()
        if bv_log:
            w = float(U.ratio(x.grad, e["g64"], e["bound"]).max())
            print("%s: dpv_expect BV_log, torch float32 is %.2f of the bound" % (U.CASE_IDS[idx], w))
            assert w <= 1.0
        else:
            assert torch.equal(x.grad, e["plain32"])


def test_every_backward_is_once_differentiable():
    """Every autograd Function of ops wraps its backward in once_differentiable: a second-order gradient through a HIP
    backward raises (test_dpv_backward_gpu.py runs it), where a plain backward's result would pass for a constant -- on a toy
    Function built the same way, d/dx sum(g) of y = x^2 with loss sum(y^2) is 0 instead of 12 x^2."""
    from pdepth_amd import ops
    fns = [f for f in vars(ops).values() if isinstance(f, type) and issubclass(f, torch.autograd.Function)]
    assert len(fns) >= 6
    for f in fns:
        assert hasattr(f.backward, "__wrapped__"), f.__name__

    def square(once):
        class Sq(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                ctx.save_for_backward(x)
                return x * x

            @staticmethod
            def backward(ctx, g):
                (x,) = ctx.saved_tensors
                return 2 * x.detach() * g

        if once:
            Sq.backward = staticmethod(torch.autograd.function.once_differentiable(Sq.backward))
        return Sq.apply

    x = torch.tensor([1.0, 2.0], requires_grad=True)
    (g,) = torch.autograd.grad((square(False)(x) ** 2).sum(), x, create_graph=True)
    (gg,) = torch.autograd.grad(g.sum(), x)
    assert torch.equal(g.detach(), 4 * x.detach() ** 3) and not torch.equal(gg, 12 * x.detach() ** 2)   # silently wrong
    (g,) = torch.autograd.grad((square(True)(x) ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
