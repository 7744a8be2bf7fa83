"""CPU only: keeps the float64 restatement and the bound of tests/util_correlation.py honest and checks what the GPU suite
(test_correlation_gpu.py) relies on -- that float32 emulations of the kernels' three summation orders (one ascending fma chain;
the matrix-pipe kernel's four interleaved chains added pairwise; the backward's ascending chain over the displacements) stay
inside the a-priori bound on every input family, that each of seven plausible kernel mistakes lands outside it at the
smallest channel count and at C = 256, that the restatement agrees with oracle.ref_cpu.correlation_general (values, gradients
and the class of every non-finite element) and with fixtures g9 / g12, and that which_kernel gives the dispatch table of the
module docstring."""
import pytest
import torch

import pdepth_amd  # noqa: F401
from oracle import ref_cpu as O
from util import golden
import util_correlation as U

FAST = ((4, 1, 4, 1, 1), (6, 1, 6, 1, 2))   # the fast configuration at stride2 1 and 2: 81 and 49 displacements
CONFIGS = [(4, 1, 4, 1, 1), (5, 1, 4, 1, 1), (3, 1, 4, 1, 2), (4, 1, 4, 2, 1), (4, 3, 4, 1, 3), (6, 3, 5, 2, 2), (20, 1, 20, 1, 2)]


def _case(family, C, cfg, seed=0, H=9, W=11):
    shape = (2, C, H, W)
    x1, x2, go = U.inputs(family, shape, cfg, 3100 + seed + C)
    return shape, x1, x2, go, U.reference(x1, x2, go, cfg)


# ---- 1. the bound is one float32 can meet -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", U.FAMILIES)
def test_float32_emulations_stay_inside_the_bound(family):
    top = {}
    for cfg in FAST:
        for C in (1, 3, 5, 17, 64, 256):
            shape, x1, x2, go, r = _case(family, C, cfg, H=7 if C > 17 else 9, W=9 if C > 17 else 11)
            md, s2 = cfg[2], cfg[4]
            for order in ("ascending", "pipe"):
                w = U.check(U.emulate_forward32(x1, x2, md, s2, order), r, "out", shape, cfg)
                top[order] = max(top.get(order, 0.0), w)
            g1, g2 = U.emulate_backward32(x1, x2, go, md, s2)
            top["g1"] = max(top.get("g1", 0.0), U.check(g1, r, "g1", shape, cfg))
            top["g2"] = max(top.get("g2", 0.0), U.check(g2, r, "g2", shape, cfg))
    print("emulation, %-11s worst err / bound: %s" % (family, ", ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    assert all(v <= 1.0 for v in top.values()), top
    assert all(v > 0.0 for v in top.values()), top   # (a float32 evaluation is not exact: the comparison sees it)


# ---- 2. the bound catches what it should --------------------------------------------------------------------------------------
MUTANT_OUTPUT = {m: ("g2" if m == "unmirrored_g2" else "out") for m in U.MUTANTS}


@pytest.mark.parametrize("C", (1, 256))
@pytest.mark.parametrize("mutant", U.MUTANTS)
def test_mutants_of_the_reference_exceed_the_bound(mutant, C):
    cfg = FAST[0]
    shape, x1, x2, go, r = _case("randn", C, cfg, seed=7)
    bad = U.reference(x1, x2, go, cfg, mutant=mutant)
    name = MUTANT_OUTPUT[mutant]
    w = U.check(bad[name], r, name, shape, cfg)
    print("mutant %-15s C = %3d: worst err / bound = %.3g" % (mutant, C, w))
    assert w > 1.0, (mutant, C, w)
    if name == "out" and mutant != "drop_channel":   # the mistake is in the gradients too (a dropped channel of x1: in d x2 only)
        assert max(U.check(bad[k], r, k, shape, cfg) for k in ("g1", "g2")) > 1.0
    # ... and in the fp16 bound of the same reference
    _, C_, H, W = shape
    E16 = U.bound(r[name], r["A_" + name], U.terms(C_, H, W, cfg, name != "out"), half=True)
    assert U.worst(bad[name], r[name], E16) > 1.0, (mutant, C)


# ---- 3. the restatement against the oracle and the fixtures --------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS)
def test_reference_is_the_oracle_in_float64(cfg):
    H, W = (13, 18) if cfg[2] < 10 else (25, 27)
    shape = (2, 6, H, W)
    x1, x2, go = U.inputs("randn", shape, cfg, 3200 + cfg[0])
    r = U.reference(x1, x2, go, cfg)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    want = O.correlation_general(a, b, *cfg)
    assert want.shape == r["out"].shape
    want.backward(go.double())
    for got, ref, A in ((r["out"], want.detach(), r["A_out"]), (r["g1"], a.grad, r["A_g1"]), (r["g2"], b.grad, r["A_g2"])):
        assert float(((got - ref).abs() - 1e-13 * A).max()) <= 0.0
    assert bool((r["A_out"] >= r["out"].abs()).all()) and bool((r["A_g1"] >= r["g1"].abs()).all())
    # float32: the oracle as the existing tests use it is inside the bound of its own order
    assert U.check(O.correlation_general(x1, x2, *cfg), r, "out", shape, cfg) <= 1.0


@pytest.mark.parametrize("cfg", CONFIGS)
def test_nonfinite_classes_are_the_padded_oracles(cfg):
    """Every element of the forward and of both gradients is finite, +inf, -inf or NaN exactly where the F.pad oracle's is
    (forward in float64 arithmetic, the gradients through its autograd: both multiply the padding's zeros)."""
    H, W = (13, 18) if cfg[2] < 10 else (25, 27)
    shape = (2, 6, H, W)
    x1, x2, go = U.plant_nonfinite(*U.inputs("randn", shape, cfg, 3300 + cfg[0]))
    r = U.reference(x1, x2, go, cfg)
    a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    want = O.correlation_general(a, b, *cfg)
    want.backward(go.double())
    for name, ref in (("out", want.detach()), ("g1", a.grad), ("g2", b.grad)):
        assert torch.equal(U.classes(r[name]), U.classes(ref)), name
        fin = torch.isfinite(ref)
        assert float((r[name][fin] - ref[fin]).abs().max()) <= 1e-12
        assert int((~fin).sum()) > 0 and (name != "out" or int((U.classes(ref) == 3).sum()) > 0), name   # (the plants reach every output)


def test_reference_matches_the_fixtures():
    cfg = (4, 1, 4, 1, 1)
    g = golden("g9_correlation.npz")
    x1, x2 = torch.from_numpy(g["x1"]), torch.from_numpy(g["x2"])
    r = U.reference(x1, x2, None, cfg)
    assert U.check(torch.from_numpy(g["out"]), r, "out", tuple(x1.shape), cfg) <= 1.0
    g = golden("g12_correlation_backward.npz")
    x1, x2, go = torch.from_numpy(g["x1"]), torch.from_numpy(g["x2"]), torch.from_numpy(g["grad_out"])
    r = U.reference(x1, x2, go, cfg)
    assert U.check(torch.from_numpy(g["grad_x1"]), r, "g1", tuple(x1.shape), cfg) <= 1.0
    assert U.check(torch.from_numpy(g["grad_x2"]), r, "g2", tuple(x1.shape), cfg) <= 1.0


# ---- 4. the dispatch table -----------------------------------------------------------------------------------------------------
def test_which_kernel_is_the_dispatch_table():
    f = lambda r, s2: (r * s2, 1, r * s2, 1, s2)
    sh = lambda C: (2, C, 9, 17)
    assert [U.which_kernel(sh(C), f(4, 1)) for C in (1, 64, 65, 128, 129, 256, 257)] == \
        [U.MFMA[16], U.MFMA[16], U.MFMA[32], U.MFMA[32], U.MFMA[64], U.MFMA[64], U.SCALAR[4]]
    assert U.which_kernel(sh(8), f(4, 4)) == U.MFMA[16] and U.which_kernel(sh(8), f(1, 17)) == U.SCALAR[1]
    assert U.which_kernel(sh(8), f(4, 36)) == U.SCALAR[4] and U.which_kernel(sh(8), f(4, 37)) == U.GENERAL
    assert U.forward_lds(48) <= U.LDS_OPT_IN < U.forward_lds(49) and U.forward_lds(144) <= U.LDS_CAP < U.forward_lds(145)
    assert U.backward_lds(8) <= U.LDS_OPT_IN < U.backward_lds(9) and U.backward_lds(17) <= U.LDS_CAP < U.backward_lds(18)
    assert [U.which_kernel(sh(8), f(r, s2), backward=True) for r, s2 in ((4, 1), (4, 2), (3, 3), (1, 17), (3, 6), (4, 5))] == \
        [U.FAST_BWD, U.FAST_BWD, U.FAST_BWD_OPT_IN, U.FAST_BWD_OPT_IN, U.GENERAL, U.GENERAL]
    for cfg in ((5, 1, 4, 1, 1), (4, 1, 4, 2, 1), (4, 3, 4, 1, 3), (20, 1, 20, 1, 2), (5, 1, 5, 1, 1)):   # pad, stride1, kernel, radius 10, radius 5
        assert U.which_kernel(sh(8), cfg) == U.GENERAL and U.which_kernel(sh(8), cfg, backward=True) == U.GENERAL
    assert U.which_kernel(sh(8), f(4, 1), half=True) == U.GENERAL and U.which_kernel(sh(8), f(4, 1), half=True, backward=True) == U.GENERAL
