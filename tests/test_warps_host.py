"""CPU only: keeps the references of tests/util_warps.py honest and checks the conditions the GPU suite (test_warps_gpu.py)
relies on -- that the cases reach what their names say, that stable_mask's delta is wide enough, that the reference's own
float32 paths stay inside the bounds the kernels are held to."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd.utils import inverse_warp as iw
from oracle import ref_cpu as O
from util import golden
import util_warps as U

WF_NAMES = [n for n, _ in U.WARP_FEATURE_CASES]
IW_NAMES = [n for n, _ in U.INVERSE_WARP_CASES]


# ---- bilinear64 / warp_feature_exact64 ---------------------------------------------------------------------------------------
def test_bilinear64_on_hand_made_positions():
    """Integer positions return the texel, half-way positions the mean, a tap outside the image counts as zero, a
    non-finite position yields the marker (never an exception), and the gather is differentiable in src."""
    src = torch.arange(12, dtype=torch.float32).reshape(1, 3, 4).requires_grad_(True)
    ix = torch.tensor([[1.0, 0.5, -0.5, 3.5, 1.25, float("nan"), float("inf"), 1e30, -1e30, 2.0]])
    iy = torch.tensor([[2.0, 0.5, 0.0, 2.5, -1.0, 0.0, 0.0, 0.0, 1.0, float("-inf")]])
    out = U.bilinear64(src, ix, iy, nonfinite=-7.0)
    want = [9.0, (0 + 1 + 4 + 5) / 4.0, 0.0, 11.0 / 4.0, 0.0, -7.0, -7.0, 0.0, 0.0, -7.0]
    assert out.dtype == torch.float64 and out.tolist()[0] == want
    assert torch.isnan(U.bilinear64(src, ix, iy)[0, 5])
    out[0, :5].sum().backward()
    g = torch.zeros(3, 4)
    g[2, 1] += 1
    g[0:2, 0:2] += 0.25
    g[0, 0] += 0.5
    g[2, 3] += 0.25
    assert torch.equal(src.grad[0], g)
    assert U.tap_mask(ix, iy, 3, 4).tolist()[0] == [1 + 2, 15, 2 + 8, 1, 4 + 8, 0, 0, 0, 0, 0]


def test_bilinear64_matches_the_reference_fixture():
    """The float64 gather at the oracle's positions against the recorded reference output (g6_warp_feature)."""
    g = golden("g6_warp_feature.npz")
    K = torch.from_numpy(g["K"])
    feat = torch.from_numpy(g["feat"])
    batch = {"src": feat, "K": K[None], "R": torch.from_numpy(g["R"])[None], "t": torch.from_numpy(g["t"])[None],
             "rays": torch.from_numpy(g["rays"])[None], "d_candi": g["d_candi"]}
    exact, fin = U.warp_feature_exact64(batch)
    assert bool(fin.all())
    # the fixture was recorded on another host: its BLAS may round K @ R @ rays differently, which moves a position by an
    # ulp (test_oracle_golden.py); the oracle on THIS host is held to the derived bound, the fixture to the suite's 1e-6
    here = U.warp_feature_oracle32(batch)
    assert bool(((here.double() - exact).abs() <= U.warp_feature_bound(feat)).all())
    np.testing.assert_allclose(exact.numpy(), g["out"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", WF_NAMES)
def test_reference_float32_warp_feature_stays_within_the_bound(name):
    """O.warp_feature, the reference's own float32 path, is within 4 eps32 max|src| of exact64 on every case (where the
    position is finite), so the bound test_warps_gpu.py holds the kernel to is one the reference itself meets."""
    b = U.warp_feature_case(name)
    exact, fin = U.warp_feature_reference(name)
    assert tuple(exact.shape) == tuple(b["src"].shape)
    got = U.warp_feature_oracle32(b)
    err = torch.where(fin, (got.double() - exact).abs(), torch.zeros_like(exact))
    bound = U.warp_feature_bound(b["src"])
    worst = float((err / bound * 4).max())
    print("%s: reference float32 path is %.2f eps32 max|src| from exact64; %d non-finite positions" % (name, worst, int((~fin).sum())))
    assert bool((err <= bound).all())
    # where the position is not finite the float32 path yields NaN or zero, never a texel
    assert bool((torch.isnan(got) | (got == 0))[~fin].all())


def test_warp_feature_cases_reach_what_they_are_named_for():
    for name, want in U.WARP_FEATURE_NCHUNK.items():
        B, V, D, H, W = U.warp_feature_case(name)["src"].shape
        assert U.launcher_nchunk(B, V, D, H, W) == want, name
    assert tuple(U.warp_feature_case("chunks16_ragged_planes")["src"].shape[2:]) == (37, 17, 23)   # HW = 391: ragged block
    oc = U.warp_feature_case("off_centre_items")
    assert len({tuple(x.tolist()) for x in oc["cxcy"]}) == 3
    # the extreme poses: taps on the border, samples outside, positions far beyond the image (none of the three produces a
    # non-finite position on these inputs: the GPU test's comparison at non-finite positions stands for inputs that do)
    for name in U.WARP_FEATURE_EXTREME:
        b = U.warp_feature_case(name)
        ix, iy = U.oracle_positions(b)
        H, W = b["src"].shape[-2:]
        m = U.tap_mask(ix, iy, H, W)
        partial = int(((m != 0) & (m != 15)).sum())
        outside = int((m == 0).sum())
        far = int((~torch.isfinite(ix) | ~torch.isfinite(iy) | (ix.abs() > 10 * W) | (iy.abs() > 10 * W)).sum())
        print("%s: %d border samples, %d outside, %d far or non-finite of %d" % (name, partial, outside, far, m.numel()))
        assert partial > 0 and outside > 0
        if name == "behind":
            assert far > 0


# ---- inverse_warp64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IW_NAMES)
@pytest.mark.parametrize("mode", U.MODES)
def test_inverse_warp64_is_the_oracle_on_doubles(name, mode):
    """The restated lines compute what O.inverse_warp computes when it is handed float64 inputs, bit for bit."""
    c = U.inverse_warp_case(name)
    r = U.inverse_warp64(c["img"], c["depth"], c["pose"], c["K"], mode, c["rot"])
    pm = U._pose_mat(c["pose"].double(), c["rot"])
    out, valid = O.inverse_warp(c["img"].double(), c["depth"].double(), pm, c["K"].double(), mode)
    assert out.dtype == torch.float64
    assert torch.equal(torch.nan_to_num(out, nan=-1e300), torch.nan_to_num(r["out"].detach(), nan=-1e300))
    assert torch.equal(valid, r["valid"])


def test_inverse_warp64_matches_the_reference_fixtures():
    """g11 (forward, three pose forms) and g17 (gradients) at the tolerances test_next_rows.py uses for the oracle on a host
    other than the fixture's."""
    g = golden("g11_inverse_warp.npz")
    t = lambda k, gg=g: torch.from_numpy(gg[k])
    for pose_key, rot, okey, vkey in (("pose44", "euler", "out44", "valid44"), ("pose6", "euler", "out6e", "valid6e"),
                                      ("pose6", "quat", "out6q", "valid6q")):
        r = U.inverse_warp64(t("img"), t("depth"), t(pose_key), t("K"), "bilinear", rot)
        np.testing.assert_allclose(r["out"].detach().numpy(), g[okey], rtol=5e-4, atol=5e-4)
        assert (r["valid"].numpy() != g[vkey]).mean() < 0.01
    g = golden("g17_inverse_warp_backward.npz")
    gout = torch.from_numpy(g["grad_out"])
    for mode in U.MODES:
        for rot in ("euler", "quat"):
            r = U.inverse_warp64(t("img", g), t("depth", g), t("pose6", g), t("K", g), mode, rot)
            q = U._grads(r, gout)
            tag = mode + "_" + rot
            np.testing.assert_allclose(q["out"].numpy(), g[tag + "_out"], rtol=1e-4, atol=2e-4)
            assert (r["valid"].numpy() != g[tag + "_valid"]).mean() < 0.01
            np.testing.assert_allclose(q["g_img"].numpy(), g[tag + "_gimg"], rtol=1e-4, atol=2e-4)
            if mode == "bilinear":
                gd, gp = g[tag + "_gdepth"], g[tag + "_gpose"]
                assert np.abs(q["g_depth"].numpy() - gd).max() <= 2e-3 * np.abs(gd).max()
                assert np.abs(q["g_pose"].numpy() - gp).max() <= 2e-3 * np.abs(gp).max()
    r = U.inverse_warp64(t("img", g), t("depth", g), t("pose44", g), t("K", g))
    q = U._grads(r, gout)
    for key, name in (("p44_gdepth", "g_depth"), ("p44_gpose", "g_pose"), ("p44_gK", "g_K")):
        assert np.abs(q[name].numpy() - g[key]).max() <= 2e-3 * np.abs(g[key]).max(), key


# ---- the cases of inverse_warp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IW_NAMES)
@pytest.mark.parametrize("mode", U.MODES)
def test_stable_mask_keeps_98_percent_and_enough_samples_inside(name, mode):
    """Uniform fractional parts predict 1 - 4 delta = 99.6 % (two coordinates, +-delta each) before the other conditions.  At
    least 30 % of the stable pixels have all four taps inside -- except in the cases named 'outside' -- so that no case
    passes on zeros."""
    ref = U.inverse_warp_reference(name, mode)
    M = ref["M"]
    expected = torch.ones_like(M)
    if name == "nan_depth":
        for (b, y, x, _) in U.NAN_DEPTH_PIXELS:
            expected[b, y, x] = False                      # a non-finite position is never stable
        assert not bool(M[~expected].any())
    kept = float(M[expected].double().mean())
    inside = float((ref["taps"][M] == 15).double().mean())
    print("%s/%s: stable_mask drops %.2f %% of the pixels; %.1f %% of the stable ones have four taps inside"
          % (name, mode, 100 * (1 - kept), 100 * inside))
    assert kept >= 0.98
    if "outside" not in name:
        assert inside >= 0.30


def test_inverse_warp_cases_reach_what_they_are_named_for():
    ref = {n: U.inverse_warp_reference(n, "bilinear") for n in IW_NAMES}
    c = U.inverse_warp_case("ragged")
    assert c["img"].shape[-2] * c["img"].shape[-1] == 2 * 256 + 1
    for k in ("K", "pose", "depth"):
        assert not torch.equal(c[k][0], c[k][1]) and not torch.equal(c[k][1], c[k][2])
    # zoom: every sample inside a 6 x 10 patch, tens of pixels per texel
    z = ref["zoom_many_to_one"]
    assert bool((z["taps"] == 15).all())
    assert float(z["ix"].max() - z["ix"].min()) < 10.5 and float(z["iy"].max() - z["iy"].min()) < 6.5
    # border: x and y are inside or outside independently, so of the 15 non-empty subsets of {nw, ne, sw, se} only 9 can
    # be a footprint's in-bounds set (the four corners, the two rows, the two columns, all four): all 9 occur, and about
    # half the pixels have some but not all taps inside
    bt = ref["border"]["taps"]
    assert {int(m) for m in bt.unique()} >= {1, 2, 4, 8, 3, 12, 5, 10, 15}
    partial = float(((bt != 0) & (bt != 15)).double().mean())
    print("border: %.1f %% of the pixels have 1..3 taps outside" % (100 * partial))
    assert 0.4 <= partial <= 0.6
    # outside_far: positions of 3e5 .. 5e6 px (fx t / depth), far beyond the [-2, size + 1] clamp, finite
    o = ref["outside_far"]
    assert float(o["ix"].abs().min()) > 1e5 and bool(torch.isfinite(o["ix"]).all()) and bool((o["taps"] == 0).all())
    for k in U.QUANTITIES:
        assert float(o["q"][k].abs().max()) == 0.0, k
    # behind: about half the pixels are behind the clamp
    bh = ref["behind"]
    share = float((bh["pz"] < 1e-3).double().mean())
    assert 0.35 <= share <= 0.6
    # nan_depth: NaN, +inf and -inf depth; the -inf one is the infinite (not NaN) position
    n = ref["nan_depth"]
    (b0, y0, x0, _), (b1, y1, x1, _), (b2, y2, x2, _) = U.NAN_DEPTH_PIXELS
    assert torch.isnan(n["ix"][b0, y0, x0]) and not torch.isfinite(n["ix"][b1, y1, x1])
    assert torch.isinf(n["ix"][b2, y2, x2]) or torch.isinf(n["iy"][b2, y2, x2])
    assert int((~torch.isfinite(n["ix"]) | ~torch.isfinite(n["iy"])).sum()) == 3


@pytest.mark.parametrize("name", IW_NAMES)
@pytest.mark.parametrize("mode", U.MODES)
def test_float32_oracle_takes_the_float64_branches_on_stable_pixels(name, mode):
    """The yardstick of the GPU bounds, and the check that stable_mask's delta is wide enough: on every stable pixel the float32
    oracle's validity equals float64's, in nearest mode so does its output (the same texel: the float32 image value exactly), and
    its distance from float64 is finite for every quantity."""
    c = U.inverse_warp_case(name)
    ref = U.inverse_warp_reference(name, mode)
    y = U.oracle32_yardstick(name, mode)
    M = ref["M"]
    assert torch.equal(y["valid32"][M], ref["valid"][M])
    if mode == "nearest":
        Mc = M.unsqueeze(1).expand_as(c["img"])
        assert torch.equal(y["q32"]["out"].double()[Mc], ref["q"]["out"][Mc])
    differ = float(((y["valid32"] != ref["valid"]) | ((y["q32"]["out"].double() != ref["q"]["out"]).any(1) & (mode == "nearest"))).double().mean())
    assert differ <= 0.02
    print("%s/%s: e_ref %s scale %s" % (name, mode, {k: "%.2e" % v for k, v in y["e_ref"].items()},
                                       {k: "%.2e" % v for k, v in y["scale"].items()}))
    for k in U.QUANTITIES:
        assert np.isfinite(y["e_ref"][k]) and np.isfinite(y["scale"][k]), k
        if mode == "nearest" and k in ("g_depth", "g_pose", "g_K"):
            assert y["e_ref"][k] == 0.0 and y["scale"][k] == 0.0
