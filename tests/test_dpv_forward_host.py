"""CPU only: keeps the float64 restatement and the bound of tests/util_dpv_forward.py honest and checks what the GPU suite
(test_dpv_forward_gpu.py) relies on -- that the restatement is float64 torch.log_softmax / softmax and the oracle's expectation
and variance, that a float32 emulation of each kernel order sits inside the a-priori bound on every case, kind and op, that
each of six plausible kernel mistakes lands at least ten times outside it on a named case and kind, that the exact
expectations hold for the emulation, and that order_of gives the table of the module docstring."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from oracle import ref_cpu as O
import util_dpv_forward as U

IDX = range(len(U.CASES))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_restatement_is_float64_log_softmax_and_the_oracle(idx):
    B, D, H, W = U.SHAPES[idx]
    dc = U.candidates(idx)
    dc64 = dc.double().numpy()
    for kind in U.kinds_for(D):
        for with_addend in (False, True):
            r = U.reference(idx, kind, with_addend)
            f, x = r["f"], r["x32"].double()
            if with_addend:   # the float32 sum is the input, not the float64 one
                assert torch.equal(r["x32"], U.logits(idx, kind) + U.addend(idx))
            lp, p = torch.log_softmax(x, 1), torch.softmax(x, 1)
            fin = torch.isfinite(lp)
            assert torch.equal(fin, torch.isfinite(f["logp"])) and torch.equal(f["logp"][~fin], lp[~fin])
            assert float((f["logp"] - lp)[fin].abs().max()) <= 1e-12
            assert float((f["prob"] - p).abs().max()) <= 1e-14
            assert f["quarter"].shape == (B, D, H // 4, W // 4)
            for b in range(B):   # the oracle handles one item at a time
                want = O.dpv_to_depthmap(f["logp"][b:b + 1], dc64, BV_log=True)[0]
                assert float((f["depth"][b] - want).abs().max()) <= 1e-12 * float(dc.max())
                mean, var = O.dpv_variance(f["logp"][b:b + 1], dc64)
                assert float((f["depth"][b] - mean).abs().max()) <= 1e-12 * float(dc.max())
                assert float((f["var"][b] - var).abs().max()) <= 1e-12 * float(dc.max()) ** 2
        for bv_log in (True, False):
            v, vol = U.volume_reference(idx, kind, bv_log), U.volume(idx, kind, bv_log)
            assert vol.dtype == torch.float32
            scale = max(1.0, float(v["z"].abs().sum(1).max()))
            for b in range(B):
                want = O.dpv_to_depthmap(vol[b:b + 1].double(), dc64, BV_log=bv_log)[0]
                assert float((v["depth"][b] - want).abs().max()) <= 1e-12 * float(dc.max()) * scale
            if bv_log:
                mean, var = O.dpv_variance(vol[:1].double(), dc64)
                assert float((v["var"][0] - var).abs().max()) <= 1e-12 * float(dc.max()) ** 2 * scale
    lin = U.volume(idx, "randn3", False)   # the linear form is held on a volume that is neither normalised nor non-negative
    assert bool((lin < 0).any()) or lin.numel() < 4
    assert float((lin.double().sum(1) - 1).abs().max()) > 1e-3


# ---- 2. a float32 evaluation in each kernel order sits inside the bound ------------------------------------------------------
def test_emulation_sits_inside_the_bound_on_every_case_kind_and_order():
    top = {}

    def note(order, name, value, where):
        if value > top.get((order, name), (-1.0, None))[0]:
            top[(order, name)] = (value, where)

    for idx in IDX:
        D = U.SHAPES[idx][1]
        dc = U.candidates(idx)
        for kind in U.kinds_for(D):
            for order in (U.LANES, U.ASCENDING):
                for with_addend in (False, True):
                    r = U.reference(idx, kind, with_addend)
                    out = U.emulate32(r["x32"], dc, order)
                    for name, w in U.check_outputs(out, r["f"], U.bound(idx, kind, with_addend, order)).items():
                        note(order, name, w, (U.CASE_IDS[idx], kind, with_addend))
                    assert U.exact_failures(r["x32"], dc, out) == 0, (U.CASE_IDS[idx], kind, order)
                for bv_log in (True, False):
                    v = U.volume_reference(idx, kind, bv_log)
                    out = U.emulate_volume32(U.volume(idx, kind, bv_log), dc, bv_log, order)
                    E = U.volume_bound(v, order)
                    for name in ("depth", "var"):
                        note(order, "%s of a %s volume" % (name, "log" if bv_log else "linear"), U.worst(out[name], v[name], E[name]),
                             (U.CASE_IDS[idx], kind))
    for (order, name), (value, where) in sorted(top.items()):
        print("emulation, %-9s order: %-26s worst err / bound = %.3f %s" % (order, name, value, where))
    assert all(value <= 1.0 for value, _ in top.values()), {k: v for k, v in top.items() if v[0] > 1.0}


@pytest.mark.parametrize("mistake", U.MISTAKES)
def test_planted_mistake_lands_outside_the_bound(mistake):
    idx, kind, order, name = U.MISTAKE_CASE[mistake]
    r = U.reference(idx, kind)
    dc = U.candidates(idx)
    E = U.bound(idx, kind, False, order)
    clean = U.worst(U.emulate32(r["x32"], dc, order)[name], r["f"][name], E[name])
    factor = U.worst(U.emulate32(r["x32"], dc, order, mistake=mistake)[name], r["f"][name], E[name])
    print("%s on %s %s (%s order): %s %.3g times the bound (clean: %.3f)" % (mistake, U.CASE_IDS[idx], kind, order, name, factor, clean))
    assert clean <= 1.0 and factor >= 10


def test_lp_fused_is_invisible_to_the_flat_tolerance_it_replaces():
    """x - (m + ls) on the `offset` kind: beyond the bound by the factor above, inside 3e-5 max(1, |x|max / 10), the tolerance
    of tests/test_ops_fuzz.py -- the gap this file closes."""
    idx, kind, order, _ = U.MISTAKE_CASE["lp_fused"]
    r = U.reference(idx, kind)
    got = U.emulate32(r["x32"], U.candidates(idx), order, mistake="lp_fused")["logp"]
    err = float((got.double() - r["f"]["logp"]).abs().max())
    assert 1e-4 < err < 3e-5 * float(r["x32"].abs().max()) / 10


# ---- 3. the tables ---------------------------------------------------------------------------------------------------------
def test_dispatch_table():
    L, A = U.LANES, U.ASCENDING
    # (reduce, reduce_ex, expect) per case, as the module docstring's table lists them
    table = [(A, A, A), (A, A, A), (L, L, L), (L, L, L), (A, A, A), (L, L, L), (L, L, L), (L, L, L), (L, L, L), (A, A, A), (A, A, A),
             (L, A, L), (A, A, A), (L, A, L)]
    assert len(table) == len(U.CASES)
    for idx, (shape, off, ipa) in enumerate(U.CASES):
        got = tuple(U.order_of(op, shape, aligned=not off, inplace_addend=ipa) for op in ("reduce", "reduce_ex", "expect"))
        assert got == table[idx], U.CASE_IDS[idx]
        assert U.order_of("moments", shape) == A
    assert U.order_of("reduce_ex", U.SHAPES[13]) == L   # without the addend the in-place call stays in the wave layout
    assert [U.order_of("reduce_ex", U.SHAPES[i], half=True) for i in U.HALF_CASES] == [L, L, L]
    assert sorted({8 if U.SHAPES[i][1] <= 32 else 16 if U.SHAPES[i][1] <= 64 else 32 for i in U.HALF_CASES}) == [8, 16, 32]
    n_old = len(U.UB.CASES)   # the added shapes are no larger than the ones the backward's table has
    assert max(int(np.prod(s)) for s in U.SHAPES[n_old:]) <= min(int(np.prod(s)) for s in U.SHAPES[3:n_old])


def test_kinds_are_what_they_claim():
    for idx in IDX:
        B, D, H, W = U.SHAPES[idx]
        hot = U.logits(idx, "one_hot")
        assert bool(((hot > float("-inf")).sum(1) == 1).all())
        neg = U.logits(idx, "offset_neg")
        assert float(neg.max()) < -9.9e3 and float(neg.min()) > -1.01e4
        if D >= 2:
            assert bool(torch.isinf(U.logits(idx, "masked")).any(1).all())
    for shape in (U.SHAPES[5], U.SHAPES[4]):
        pix = [p for _, p in U.nonfinite_pixels(shape)]
        HW = shape[2] * shape[3]
        assert 0 in pix and HW - 1 in pix and {p % 4 for p in pix} == {0, 1, 2, 3} and any(p >= 64 * ((HW - 1) // 64) for p in pix)
