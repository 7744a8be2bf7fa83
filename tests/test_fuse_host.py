"""CPU only: keeps the float64 restatement and the bound of tests/util_fuse.py honest and checks what the GPU suite
(test_fuse_gpu.py) relies on -- that the restatement is the oracle's dpv_fuse and the fixture's, that its gradient is float64
autograd's, that a float32 evaluation of the kernels' loops sits inside the a-priori bound on every case, that each of seven
plausible kernel mistakes fails the same comparison by a factor of ten or more on a named case, and that no generated column
lies in the band where the value is not pinned."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from oracle import ref_cpu as O
from util import golden
import util_fuse as U

IDX = range(len(U.CASES))


def _emulated(idx, mode=None, mistake=None):
    def make():
        c = U.case(idx)
        g_f, g_l = U.grads_of(c, mode) if mode else (None, None)
        return U.emulate32(c["logp"], c["dmaps"], c["masks"], c["dc"], g_f, g_l, mistake=mistake)
    return U.cached(("emu", idx, mode, mistake), make)


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_restatement_is_the_oracle_on_normal_and_dead_columns(idx):
    """O.dpv_fuse in float32 against forward64: inside the bound (the oracle is one more float32 evaluation) on every plane."""
    c = U.case(idx)
    fused, logf = O.dpv_fuse(c["logp"], c["dmaps"], c["masks"].unsqueeze(1), c["dc"].numpy(), U.VAR)
    rf, rl = U.check_forward(idx, fused, logf)
    print("%s: oracle float32 against the restatement: fused %.3f, log fused %.3f of the bound" % (U.CASE_IDS[idx], rf, rl))
    assert rf <= 1 and rl <= 1


def test_restatement_is_the_fixture():
    g = golden("g10_dpv_fuse.npz")
    logp, dm, mk = (torch.from_numpy(g[k]) for k in ("logp", "dmaps", "masks"))
    dc = torch.from_numpy(np.asarray(g["d_candi"], dtype=np.float32))
    f = U.forward64(logp, dm, mk[:, 0], dc)
    assert int(f["band"].sum()) == 0 and bool(f["normal"].all())
    E = U.forward_bound(f)
    rf = float(U.ratio(torch.from_numpy(g["fused"]), f["fused"], E["fused"]).max())
    rl = float(U.ratio(torch.from_numpy(g["logfused"]), f["logf"], E["logf"]).max())
    rm = float((torch.from_numpy(g["tofuse"]).double() - f["m"]).abs().max())
    print("fixture against the restatement: fused %.3f, log fused %.3f of the bound; prior %.2e" % (rf, rl, rm))
    assert rf <= 1 and rl <= 1 and rm <= 1e-6


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_closed_form_is_float64_autograd_away_from_the_clamp(idx, mode):
    from test_fuse_backward import fuse_torch
    c, r = U.case(idx), U.reference(idx)
    g_f, g_l = U.grads_of(c, mode)
    x = c["logp"].double().requires_grad_(True)
    # (fuse_torch forms two_var in the dtype of x: half the float32 two_var makes its float64 one the operation's)
    q, fused, logf = fuse_torch(x, c["dmaps"], c["masks"], c["dc"], U.two_var32(U.VAR) / 2, U.EPS)
    total = 0
    if g_f is not None:
        total = total + (fused * g_f.double()).sum()
    if g_l is not None:
        total = total + (logf * g_l.double()).sum()
    total.backward()
    f = r["f"]
    # autograd's own forward: the same float64 formula except on dead columns, where it divides where the rule says -1
    live = (~f["dead"]).expand_as(f["q"])
    assert float((q.detach() - f["q"]).abs()[live].max() if bool(live.any()) else 0.0) <= 1e-12
    passk = (f["q"] >= U.EPS) & (f["q"] <= 1.0)
    want = U.grad64(f, g_f, g_l, passk)
    away = ((f["q"] / U.EPS - 1).abs() > 1e-6).all(1, keepdim=True).expand_as(want) & live
    # where a column has every plane at -inf but some, or q = 1 exactly, autograd agrees too; NaN appears nowhere
    err = (x.grad - want).abs()[away]
    assert bool(torch.isfinite(x.grad[away]).all())
    scale = float(want.abs()[away].max()) if err.numel() else 0.0
    print("%s %s: closed form against float64 autograd %.2e (max |g| %.2e) on %d of %d elements"
          % (U.CASE_IDS[idx], mode, float(err.max()) if err.numel() else 0.0, scale, int(away.sum()), away.numel()))
    assert err.numel() == 0 or float(err.max()) <= 1e-12 * max(scale, 1.0)


# ---- 2. a float32 evaluation sits inside the bound -------------------------------------------------------------------------
def test_emulation_sits_inside_the_bound_on_every_case():
    worst = {"fused": 0.0, "logf": 0.0, "grad": 0.0}
    for idx in IDX:
        for mode in U.MODES:
            fused, logf, g = _emulated(idx, mode)
            rf, rl = U.check_forward(idx, fused, logf)
            rg = U.check_backward(idx, mode, g, fused)
            print("%s %s: emulation fused %.3f, log fused %.3f, gradient %.3f of the bound" % (U.CASE_IDS[idx], mode, rf, rl, rg))
            worst = {"fused": max(worst["fused"], rf), "logf": max(worst["logf"], rl), "grad": max(worst["grad"], rg)}
    print("worst emulation ratio: fused %.3f, log fused %.3f, gradient %.3f" % (worst["fused"], worst["logf"], worst["grad"]))
    assert max(worst.values()) <= 1


@pytest.mark.parametrize("mistake", [m for m in U.MISTAKES if m != "nan_to_zero"])
def test_planted_mistake_fails_the_comparison(mistake):
    idx, mode, where = U.MISTAKE_CASE[mistake]
    fused, logf, g = _emulated(idx, mode, mistake)
    if where == "forward":   # log fused: its bound is nowhere 0 (fused's is, where q lies so far below eps that eps is the only answer)
        factor = U.check_forward(idx, fused, logf)[1]
    else:   # pass_k inside the margin comes from the clean forward: the mistakes of the backward leave the forward alone
        factor = U.check_backward(idx, mode, g, _emulated(idx, mode)[0])
    print("%s on %s %s: %s %.3g times the bound" % (mistake, U.CASE_IDS[idx], mode, where, factor))
    assert factor >= 10


def test_the_value_given_to_a_nan_prior_cannot_show():
    """NaN arises from 0 / 0 alone, on every plane of a dead column at once, and a prior that is the same on every plane
    cancels in the renormalisation: -1, 0 or any other constant give softmax(x) -- at every mask, clamped to eps or not.  So
    the comparison cannot tell 0 from -1 (this planted mistake stays inside the bound), and what the dead columns pin is the
    kernels' result there, softmax(x) clamped (test_fuse_gpu.py::test_dead_columns)."""
    for idx in (0, 3, 7):
        fused, logf, _ = _emulated(idx, "both", "nan_to_zero")
        assert max(U.check_forward(idx, fused, logf)) <= 1


# ---- 3. the classifier and the generators ----------------------------------------------------------------------------------
def test_no_generated_column_is_in_the_band_and_every_kind_is_dealt():
    dealt = set()
    for idx in IDX:
        c, r = U.case(idx), U.reference(idx)
        assert r["n_band"] == 0 and bool(r["held"].all())
        dealt |= {k for k, v in c["kinds"].items() if v}
        f = r["f"]
        for kind in U.DEAD_KINDS:
            for (b, y, x) in c["kinds"][kind]:
                assert bool(f["dead"][b, 0, y, x]) and bool((f["m"][b, :, y, x] == U.EPS).all())
        for (b, y, x) in c["kinds"]["edge_normal"]:
            assert U.NORMAL_S <= float(f["S"][b, 0, y, x]) < 8 * U.NORMAL_S
        for (b, y, x) in c["kinds"]["peaked_disagree"]:
            if c["shape"][1] > 2:
                assert float(f["q"][b, :, y, x].max()) > 0.99 and int((f["q"][b, :, y, x] < U.EPS).sum()) >= 1
        cols = [f["fused"][b, :, y, x] for k in ("shifted_base", "shifted_p30", "shifted_m30") for (b, y, x) in c["kinds"][k]]
        for col in cols[1:]:   # the shift cancels: one result, while the kernels' exp sees arguments near +30 and near -100
            assert float((col - cols[0]).abs().max()) <= 1e-12
        n = c["shape"][0] * c["shape"][2] * c["shape"][3]
        if n >= len(U.KINDS):
            assert all(c["kinds"][k] for k in U.KINDS), U.CASE_IDS[idx]
    assert dealt == set(U.KINDS)
    for D in (64, 128):
        lad = U.ladder(D)
        f = U.forward64(lad["logp"], lad["dmaps"], lad["masks"], lad["dc"])
        assert bool(f["normal"].all())
        above = (f["q"][0, 1:] > U.EPS).reshape(D - 1, -1)
        crossing = int((above.any(1) & ~above.all(1)).sum())
        print("ladder D = %d: %d of %d planes cross q = eps in float64" % (D, crossing, D - 1))
        assert crossing >= (D - 1) // 3
        assert float((f["q"][0, 1:] * D).max()) <= 200 * 2.0 ** -52


def test_band_of_the_projects_candidates():
    """powerf(5, 40, 64, 1) with var 0.3: S64 < 2^-100 from 6.45 m beyond the last candidate (69.3 * 0.6 = 6.45^2), every
    argument below -110 from 8.13 m (110 * 0.6 = 8.124^2): the band is 46.45 ... 48.13 above and -3.13 ... -1.45 below."""
    dc = U.candidates(64)
    d = torch.arange(-60.0, 110.0, 0.01).view(1, 1, -1)
    normal, dead, band = U.classify(d, dc)
    inside = d[band]
    assert inside.numel() > 0
    assert bool((((inside > 46.44) & (inside < 48.13)) | ((inside > -3.13) & (inside < -1.44))).all())
    assert bool(band[(d > 46.46) & (d < 48.12)].all()) and bool(band[(d > -3.12) & (d < -1.46)].all())
    assert bool(normal[(d > -1.4) & (d < 46.4)].all()) and bool(dead[(d > 48.2) | (d < -3.2)].all())


@pytest.mark.parametrize("depth", [47.3, 47.8, -2.5])
def test_generator_refuses_a_band_depth(depth):
    with pytest.raises(ValueError, match="band"):
        U.checked_depth(depth, U.candidates(64))
    assert U.checked_depth(46.4, U.candidates(64)) == pytest.approx(46.4) and U.checked_depth(1000.0, U.candidates(64)) == 1000.0
