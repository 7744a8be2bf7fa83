"""CPU only: keeps the float64 restatement and the bounds of tests/util_soft_ce.py honest and checks what the GPU suite
(test_soft_ce_gpu.py) relies on -- that float32 emulations of the kernels' two summation orders stay inside the a-priori bounds
on every input family (and are not exact: the comparison sees a float32 error), that each of twelve plausible kernel mistakes
lands outside the bound of the output it corrupts at the smallest D of the suite at which it is a different program and at
D = 130, that the restatement agrees with fixture g24 (the reference's float32 values: loss, gradient and the from-depth label)
within the bounds of an arbitrary summation order and with the gen_soft_label_torch + torch composition in float64, that no
generator of the suite leaves a pixel inside the underflow band, and that which_path gives this dispatch table:

    H W        D     pointers              forward and backward
    108, 260   1 .. 32    all 16-byte aligned   vec8
    108, 260   33 .. 64   all 16-byte aligned   vec16
    108, 260   65 .. 128  all 16-byte aligned   vec32
    108        129, 130   all 16-byte aligned   scalar   (D > 128)
    63, 257    any        all 16-byte aligned   scalar   (H W % 4 != 0)
    108        64         logp | label | depth_gt | mask | g_depth one float into its buffer, the others aligned   scalar
"""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from util import golden
import util_loss as UL
import util_soft_ce as U

FORMS = ("label", "depth")


def _ratios(got, r, E, names):
    return {k: U.worst(got[k], r[k], E[k]) for k in names}


# ---- 1. the bounds are ones float32 can meet -------------------------------------------------------------------------------------
EMU_SHAPES = (("vec4", "vec8", (3, 5, 9, 12)), ("vec4", "vec16", (3, 33, 13, 20)), ("vec4", "vec32", (3, 128, 9, 12)),
              ("scalar", "scalar", (3, 20, 7, 9)), ("scalar", "scalar", (3, 3, 1, 257)))


@pytest.mark.parametrize("family,form", [(fa, fo) for fa in U.VOLUMES + U.NONFINITE for fo in FORMS] + [("badz", "depth")])
def test_float32_emulations_stay_inside_the_bounds(family, form):
    top = {}
    for i, (order, path, shape) in enumerate(EMU_SHAPES):
        for j, (var, pw) in enumerate(U.DEPTH_FORMS if form == "depth" else ((0.3, 2.0),)):
            mask_kind = "binary" if family in U.NONFINITE else U.MASKS[(i + j) % 4]
            c = U.make_case(family, form, shape, 5100 + 10 * i + j, mask_kind, var, pw)
            r = U.case_reference(c)
            E = U.bound(r, path)
            got = U.emulate32(c, order)
            assert torch.equal(got["count"].double(), r["count"]), (family, form, shape)
            for k, w in _ratios(got, r, E, ("ce", "depth", "loss", "g_logp")).items():
                top[k] = max(top.get(k, 0.0), w)
                assert w <= 1.0, (family, form, order, shape, var, pw, k, w)
            if family in U.NONFINITE or family == "badz":
                assert torch.equal(U.classes(got["ce"]), U.classes(r["ce"]))
    print("emulation, %-16s %-5s worst err / bound: %s" % (family, form, ", ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    assert all(v > 0.0 for v in top.values()), top


def test_nonfinite_families_hold_what_they_say():
    for form in FORMS:
        r = U.case_reference(U.make_case("nonfinite", form, (2, 16, 9, 12), 5200))
        assert bool((r["ce"][0] == float("inf")).any()) and float(r["loss"][0]) == float("inf")
        assert bool(r["loss"][1].isnan()) == (form == "label") and bool(r["ce"][1].isnan().any()) == (form == "label")
        r = U.case_reference(U.make_case("nonfinite_masked", form, (2, 16, 9, 12), 5200))
        assert bool((r["ce"][0] == float("inf")).any()) and bool(torch.isfinite(r["loss"]).all()) and bool(torch.isfinite(r["g_logp"]).all())
    c = U.make_case("badz", "depth", (2, 16, 9, 12), 5201)
    r = U.case_reference(c)
    assert bool(r["minus"].view(2, -1)[0, 7]) and bool(r["minus"].view(2, -1)[1, 9]) and bool((r["label"].view(2, 16, -1)[0, :, 7] == -1).all())
    assert bool(torch.isfinite(r["ce"]).all())
    lab = U.make_case("soft2", "label", (2, 16, 9, 12), 5202)["label"]
    assert int((lab == 0).sum()) > 0 and bool((lab.view(2, 16, -1)[0, :, 1] == -1).all())
    m = U.make_case("soft2", "label", (3, 4, 9, 12), 5203, "values")["mask"]
    assert {0.0, 0.5, 1.0, 2.0} == set(m.unique().tolist())
    assert float(U.make_case("soft2", "label", (3, 4, 9, 12), 5203, "zero_item")["mask"][2].abs().max()) == 0.0


# ---- 2. the bounds catch what they should ------------------------------------------------------------------------------------------
# the smallest D of the suite at which the mistake is another program: group_sum's second half holds planes 2, 3, 6, 7 ...; the
# pairing (4 g + i) % D is the identity up to D = 4
MUTANT_MIN_D = {"half_group_sum": 3, "wrong_pairing": 5}


@pytest.mark.parametrize("largest", (False, True), ids=("smallest", "largest"))
@pytest.mark.parametrize("mutant", sorted(U.MUTANTS))
def test_mutants_of_the_reference_exceed_the_bound(mutant, largest):
    name, needs = U.MUTANTS[mutant]
    D = 130 if largest else MUTANT_MIN_D.get(mutant, min(U.PROBE_D))
    path = U.SCALAR if largest else "vec8"
    assert D in U.PROBE_D + U.SCALAR_D
    family, mask_kind, pw = "soft2", "none", 2.0
    if mutant in ("count_nonzero", "coef_ignores_mask_value"):
        mask_kind = "values"
    if mutant == "mask_multiplied":
        family, mask_kind = "nonfinite_masked", "binary"
    if mutant == "pow_ignored":
        pw = 3.0
    for form in FORMS if needs is None else (needs,):
        c = U.make_case(family, form, (2, D, 8, 8) if largest else (2, D, 9, 12), 5300 + D, mask_kind, 0.3, pw)
        r = U.case_reference(c)
        bad = U.case_reference(c, mutant=mutant)
        w = U.worst(bad[name], r[name], U.bound(r, path)[name])
        print("mutant %-24s %-5s D = %3d: worst err / bound of %s = %.3g" % (mutant, form, D, name, w))
        assert w > 1.0, (mutant, form, D, w)
        if mutant == "count_nonzero":
            assert not torch.equal(bad["count"], r["count"])


# ---- 3. the restatement against the fixture and the torch composition --------------------------------------------------------------
def test_reference_matches_fixture_g24():
    """ce_*, ce_zero_*, ce_*_grad_* (the reference's soft_cross_entropy_loss per item, float32, and its autograd) and label_*_lo
    (its gen_soft_label_torch): inside the bounds of a float32 evaluation in any order."""
    g = golden("g24_loss.npz")
    inp = UL.make_inputs()
    dc = torch.tensor(UL.d_candi(), dtype=torch.float32)
    ones = torch.ones(UL.B)
    for s in UL.SIDES:
        logp, label = torch.from_numpy(inp[f"logp_{s}_lo"]), torch.from_numpy(g[f"label_{s}_lo"])
        for tag, mask in (("", torch.from_numpy(inp[f"mask_{s}_lo"])[:, 0]), ("_zero", torch.zeros(UL.B, *UL.LO))):
            r = U.reference(logp, dc, label=label, mask=mask, g_loss=ones)
            E = U.bound(r, "any")
            loss = torch.tensor([float(g[f"ce{tag}_{s}_{i}"]) for i in range(UL.B)])
            grad = torch.from_numpy(np.concatenate([g[f"ce{tag}_grad_{s}_{i}"] for i in range(UL.B)]))
            w = (U.worst(loss, r["loss"], E["loss"]), U.worst(grad, r["g_logp"], E["g_logp"]))
            print("g24 %s%s: loss %.3f, gradient %.3f of the bound" % (s, tag, *w))
            assert max(w) <= 1.0, (s, tag, w)
            if tag == "_zero":
                assert float(r["loss"].abs().max()) == 0.0 and float(r["g_logp"].abs().max()) == 0.0
        r = U.reference(logp, dc, depth_gt=torch.from_numpy(inp[f"dmap_{s}_lo"]), variance=UL.VARIANCE)
        assert torch.equal(label == -1, r["label"] == -1) and torch.equal((label == -1).all(1), r["minus"])
        w = U.worst(label, r["label"], U.bound(r, "any")["label"])
        print("g24 %s: from-depth label %.3f of the bound" % (s, w))
        assert w <= 1.0
    assert float(g["ce_left_1"]) == 0.0 and int((torch.from_numpy(g["label_right_lo"]) == -1).sum()) > 0


@pytest.mark.parametrize("pw", (2.0, 3.0))
def test_reference_is_the_torch_composition_in_float64(pw):
    """gen_soft_label_torch on float64 inputs, -(label logp).sum(1), the masked mean: to 1e-13 of the sums of magnitudes.  (z stays
    inside [4, 42]: a float64 Gaussian does not underflow there, and no label is -1.)"""
    from pdepth_amd.utils import img_utils
    c = U.make_case("soft2", "depth", (2, 33, 9, 12), 5400, "values", 0.3, pw, edges=False)
    r = U.case_reference(c, grads="loss")
    assert not bool(r["minus"].any())
    var64 = torch.tensor(U.f32(0.3), dtype=torch.float64)
    v = c["logp"].double().requires_grad_(True)
    lab = torch.stack([img_utils.gen_soft_label_torch(c["dc"].tolist(), c["depth_gt"][i].double(), var64, zero_invalid=True, pow=pw)
                       for i in range(2)])
    assert lab.dtype == torch.float64 and float((lab - r["label"]).abs().max()) <= 1e-13
    ce = -(lab * v).sum(1)
    m = c["mask"].double()
    loss = (ce * m).sum((1, 2)) / (m == 1).sum((1, 2))
    (loss * c["g_loss"].double()).sum().backward()
    assert float(((ce.detach() - r["ce"]).abs() - 1e-13 * r["A_ce"]).max()) <= 0.0
    assert float(((loss.detach() - r["loss"]).abs() - 1e-13 * r["A_loss"]).max()) <= 0.0
    assert float(((v.grad - r["g_logp"]).abs() - 1e-13 * r["g_logp"].abs()).max()) <= 1e-300
    assert bool((r["A_ce"] >= r["ce"].abs() * (1 - 1e-12)).all())


# ---- 4. the condition on the inputs ---------------------------------------------------------------------------------------------------
def test_no_generator_leaves_a_pixel_inside_the_band():
    total = redrawn = 0
    for var, pw in U.DEPTH_FORMS:
        for D in U.PROBE_D + U.SCALAR_D + (8, 16, 20):
            for hw in U.PROBE_HW + U.SCALAR_HW:
                dc = U.candidates(D)
                shape = (2, D, *hw)
                z = U.depth_maps(shape, dc, var, pw, torch.Generator().manual_seed(5500 + D))
                S = torch.exp(-U.gauss64(dc, z, var, pw)).sum(1)
                assert int(U.in_band(S).sum()) == 0, (var, pw, D, hw)
                raw = 4.0 + 38.0 * torch.rand(2, *hw, generator=torch.Generator().manual_seed(5500 + D))
                redrawn += int(U.in_band(torch.exp(-U.gauss64(dc, raw, var, pw)).sum(1)).sum())
                total += z.numel()
    print("band [2^-160, 2^-116]: 0 of %d pixels inside; %d of the first draws were, and were drawn again" % (total, redrawn))
    assert redrawn > 0   # (the condition is not vacuous)
    for family in U.NONFINITE + ("badz",):
        c = U.make_case(family, "depth", (2, 8, 9, 12), 5501, "binary", 0.01, 2.0)
        S = U.case_reference(c)["S"]
        assert int(U.in_band(S).sum()) == 0
    inp = UL.make_inputs()
    dc = torch.tensor(UL.d_candi(), dtype=torch.float32)
    for s in UL.SIDES:
        for res in ("lo", "hi"):
            S = torch.exp(-U.gauss64(dc, torch.from_numpy(inp[f"dmap_{s}_{res}"]), UL.VARIANCE, 2.0)).sum(1)
            assert int(U.in_band(S).sum()) == 0
    # variance 0.01 at D = 8 puts -1 pixels inside the candidate range, and the reference refuses a map with a pixel in the band
    dc = U.candidates(8)
    z = U.depth_maps((2, 8, 13, 20), dc, 0.01, 2.0, torch.Generator().manual_seed(1))
    S = torch.exp(-U.gauss64(dc, z, 0.01, 2.0)).sum(1)
    inside = (z > 5) & (z < 40) & ~(S > U.BAND_HI)
    assert int(inside.sum()) > 20 and int((S > U.BAND_HI).sum()) > 20
    z[0, 0, 0] = float(dc[3]) + 1.4   # arg = 1.4^2 / 0.02 = 98: exp(-98) = 2^-141
    with pytest.raises(AssertionError, match="band"):
        U.reference(torch.zeros(2, 8, 13, 20), dc, depth_gt=z, variance=0.01)


# ---- 5. the dispatch table --------------------------------------------------------------------------------------------------------------
def _off_by_one_float(shape):
    """A contiguous tensor of `shape` one float into a larger buffer: its pointer is 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 4)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + n].view(shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def test_which_path_is_the_dispatch_table():
    def tensors(shape, form="label", mask=True, gd=False, off=None):
        B, D, H, W = shape
        make = lambda name, s: _off_by_one_float(s) if off == name else torch.zeros(s)
        return [make("logp", shape), make("label", shape) if form == "label" else make("depth_gt", (B, H, W)),
                make("mask", (B, H, W)) if mask else None, make("g_depth", (B, H, W)) if gd else None]
    want = {1: "vec8", 3: "vec8", 4: "vec8", 5: "vec8", 32: "vec8", 33: "vec16", 64: "vec16", 65: "vec32", 100: "vec32", 127: "vec32",
            128: "vec32", 129: "scalar", 130: "scalar"}
    assert set(want) == set(U.PROBE_D + U.SCALAR_D)
    for D, path in want.items():
        for hw in U.PROBE_HW:
            for form in FORMS:
                for gd in (False, True):
                    assert U.which_path((2, D, *hw), tensors((2, D, *hw), form, gd=gd)) == path, (D, hw, form)
        for hw in U.SCALAR_HW + ((1, 1), (3, 2)):
            assert U.which_path((2, D, *hw), tensors((2, D, *hw))) == "scalar"
    assert [U.planes_per_lane(D) for D in (1, 32, 33, 64, 65, 128)] == [8, 8, 16, 16, 32, 32]
    shape = (2, 64, 9, 12)
    assert U.which_path(shape, tensors(shape, "label", gd=True)) == "vec16"
    for form, names in (("label", ("logp", "label", "mask", "g_depth")), ("depth", ("logp", "depth_gt", "mask", "g_depth"))):
        for off in names:
            assert U.which_path(shape, tensors(shape, form, gd=True, off=off)) == "scalar", (form, off)
    assert U.which_path(shape, tensors(shape, "label", mask=False)) == "vec16"
    # the chains behind the bounds
    assert [U.chain(D, "vec8") for D in (1, 4, 5, 32)] == [3, 3, 4, 10] and U.chain(128, "vec32") == 34 and U.chain(130, "scalar") == 130
    assert U.tree(108, "vec8") == 11 and U.tree(108, "any") == 109
