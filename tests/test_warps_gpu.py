"""warp_feature (csrc/warp.hip) and inverse_warp forward + backward (csrc/inverse_warp.hip, utils/inverse_warp.py) against the
float64 references of tests/util_warps.py, on the shapes and poses where such kernels go wrong.

warp_feature: |got - exact64| <= 4 eps32 max|src[b, v]| wherever the oracle's position is finite (the derivation is in
util_warps.warp_feature_bound; test_warps_host.py shows the reference's own float32 path inside it).  A wrong tap or weight is
off by about |src|, a million times the bound.

inverse_warp: on the pixels of util_warps.stable_mask (where float32 and float64 take the same branches) the validity and the
nearest-mode output equal float64's exactly, and out, g_img, g_depth, g_pose, g_K are within max(f e_ref, 4 eps32 max|f64|) of
float64, e_ref being the distance of the reference's own float32 path (O.inverse_warp under autograd on the CPU) from float64
for the same case and quantity.  Both are float32 evaluations of one chain with differently ordered roundings (fma chain and
GPU matrix products against BLAS), and the maximum of a few thousand samples of one fluctuates by a small factor against the
other: hence the 4.  A wrong sign, a missing gZ term, another item's matrix or a lost atomic shows at about max|f64|.
g_pose and g_K are the exception: they have at most 16 entries per item, so e_ref is the maximum of a handful of numbers,
not of thousands, and an honest kernel needed 6.65 e_ref (nan_depth, g_K: only item 1's nine entries are finite and
compared; its error is 5.6e-6 of max|f64|, like every other case's).  These two are held to 16 e_ref, the others to 4.

Measured on an MI355X (printed by the tests, -s):
  warp_feature, worst |got - exact64| in units of eps32 max|src|: chunks_clamped_to_D 0.46, chunks16_ragged_planes 0.83,
    chunks3 0.96, one_chunk 0.82, model_shape 0.75, D128 0.64, off_centre_items 0.72, wide 0.71, big_rotation 0.73,
    behind 1.08, strided_views 0.65; the same with src * 16.  (The reference's float32 path: 0.46 ... 1.08.)
  inverse_warp bilinear, worst err / e_ref over the cases: out 1.11, g_img 1.32, g_depth 1.76, g_pose 2.91, g_K 6.65;
    nearest: g_img 1.22, everything else exact.  zoom_many_to_one: the sum of g_img is 2.6e-5 off 1.25e3 (bound 6.0e-4).
  pixels stable_mask drops, bilinear / nearest in %: smallest 0 / 0, ragged 0.26 / 0.32, rot_euler 0.62 / 0.62,
    rot_quat 0.45 / 0.71, zoom_many_to_one 0.10 / 0.42, border 1.04 / 0, outside_far 0 / 0, behind 1.39 / 0.93,
    nan_depth 0.72 / 0 (besides its three non-finite pixels).
  nan_depth, item 0, bilinear: out is non-finite at the three pixels (9 values), g_depth at one of them, g_img nowhere;
    12 of the 16 entries of g_pose (all of the top three rows) and all 9 of g_K are non-finite.  nearest: none.
"""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops
from pdepth_amd.utils import inverse_warp as iw
import util_warps as U
from util_warps import EPS32

pytestmark = pytest.mark.gpu

WF_NAMES = [n for n, _ in U.WARP_FEATURE_CASES]
IW_NAMES = [n for n, _ in U.INVERSE_WARP_CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- warp_feature ----------------------------------------------------------------------------------------------------------
def _warp(b, dev, src):
    t = lambda k: b[k].to(dev)
    return ops.warp_feature(src, t("K"), t("R"), t("t"), t("rays"), t("cxcy"), b["d_candi"]).cpu()


def _assert_warp(name, got, exact, fin, src, scale=1.0):
    err = torch.where(fin, (got.double() - exact * scale).abs(), torch.zeros_like(exact))
    bound = U.warp_feature_bound(src) * scale
    print("%s x%g: worst |got - exact64| = %.2f eps32 max|src|" % (name, scale, float((err / bound * 4).max())))
    assert not bool(torch.isnan(got)[fin].any())
    assert bool((err <= bound).all()), "%s: %d elements beyond 4 eps32 max|src|" % (name, int((err > bound).sum()))


@pytest.mark.parametrize("name", WF_NAMES)
def test_warp_feature_against_exact64(dev, name):
    b = U.warp_feature_case(name)
    exact, fin = U.warp_feature_reference(name)
    B, V, D, H, W = b["src"].shape
    if name in U.WARP_FEATURE_NCHUNK:
        assert U.launcher_nchunk(B, V, D, H, W) == U.WARP_FEATURE_NCHUNK[name]
    for scale in (1.0, 16.0):
        src = b["src"] * scale
        if name == "strided_views":   # the sources are the leading views of one [B,V+1,D,H,W] tensor (models/models.py:533-534)
            allv = torch.cat([src, b["ref"][:, None]], dim=1).to(dev)
            view = allv[:, :-1]
            assert not view.is_contiguous()
            got = _warp(b, dev, view)
        else:
            got = _warp(b, dev, src.to(dev))
        assert got.shape == (B, V, D, H, W)
        _assert_warp(name, got, exact, fin, b["src"], scale)
        if name in U.WARP_FEATURE_EXTREME and scale == 1.0:
            # where the position is not finite the output is the reference's own (NaN or zero)
            want = U.cached(("wf32", name), lambda: U.warp_feature_oracle32(b))
            np.testing.assert_array_equal(got[~fin].numpy(), want[~fin].numpy())


def test_warp_feature_expanded_view_equals_its_copy(dev):
    """src[:, :1].expand(-1, 2, ...): view stride 0, which _native.warp_feature materialises.  Bit for bit the result on the
    copy, and view 0 gathered at each view's own positions."""
    b = U.warp_feature_case("strided_views")
    first = b["src"][:, :1].to(dev)
    expanded = first.expand(-1, 2, -1, -1, -1)
    assert expanded.stride(1) == 0
    got = _warp(b, dev, expanded)
    assert torch.equal(got, _warp(b, dev, expanded.contiguous()))
    rep = b["src"][:, :1].expand(-1, 2, -1, -1, -1).contiguous()
    exact, fin = U.warp_feature_exact64(b, src=rep)
    _assert_warp("expanded", got, exact, fin, rep)


def test_warp_feature_does_not_depend_on_the_chunk_count(dev):
    """chunks16_ragged_planes runs with nchunk = 16; the same item repeated along B until pixblocks V B > 1024 runs with
    nchunk = 1: item 0 of that is bit-identical, and so is the last item."""
    b = U.warp_feature_case("chunks16_ragged_planes")
    _, V, D, H, W = b["src"].shape
    pixblocks = (H * W + 255) // 256
    rep = 1024 // (pixblocks * V) + 1
    assert U.launcher_nchunk(1, V, D, H, W) == 16 and U.launcher_nchunk(rep, V, D, H, W) == 1
    one = _warp(b, dev, b["src"].to(dev))
    big = {k: (v.expand(rep, *v.shape[1:]).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    many = _warp(big, dev, big["src"].to(dev))
    assert torch.equal(many[0], one[0]) and torch.equal(many[rep - 1], one[0])


# ---- inverse_warp ----------------------------------------------------------------------------------------------------------
def _hip(c, mode, dev, gup, need=("img", "depth", "pose", "K"), depth=None):
    """iw.inverse_warp under autograd on the device -> the five quantities and valid on the CPU (None: not requested)."""
    t = {k: (depth if k == "depth" and depth is not None else c[k]).to(dev).clone().requires_grad_(k in need)
         for k in ("img", "depth", "pose", "K")}
    out, valid = iw.inverse_warp(t["img"], t["depth"], t["pose"], t["K"], mode, c["rot"])
    assert out.requires_grad and not valid.requires_grad and valid.dtype == torch.bool
    (out * gup.to(dev)).sum().backward()
    g = lambda k: None if t[k].grad is None else t[k].grad.cpu()
    return {"out": out.detach().cpu(), "valid": valid.cpu(), "g_img": g("img"), "g_depth": g("depth"), "g_pose": g("pose"),
            "g_K": g("K")}


def _hip_cached(name, mode, dev):
    ref = U.inverse_warp_reference(name, mode)
    return U.cached(("iwhip", name, mode), lambda: _hip(U.inverse_warp_case(name), mode, dev, ref["gup"]))


@pytest.mark.parametrize("name", IW_NAMES)
@pytest.mark.parametrize("mode", U.MODES)
def test_inverse_warp_against_float64(dev, name, mode):
    c = U.inverse_warp_case(name)
    ref = U.inverse_warp_reference(name, mode)
    got = _hip_cached(name, mode, dev)
    M = ref["M"]
    # the branches: validity, and in nearest mode the texel, are float64's on every stable pixel
    assert torch.equal(got["valid"][M], ref["valid"][M])
    differ = got["valid"] != ref["valid"]
    if mode == "nearest":
        Mc = M.unsqueeze(1).expand_as(c["img"])
        assert torch.equal(got["out"].double()[Mc], ref["q"]["out"][Mc])
        differ = differ | (torch.nan_to_num(got["out"].double(), nan=1e300) != torch.nan_to_num(ref["q"]["out"], nan=1e300)).any(1)
    assert float(differ.double().mean()) <= 0.02
    y = U.oracle32_yardstick(name, mode)
    for k in U.QUANTITIES:
        want = ref["q"][k]
        m = U.element_mask(k, M, want)
        err, bound = U.masked_err(got[k], want, m), U.inverse_warp_bound(name, mode, k)
        print("%s/%s %s: err %.2e, e_ref %.2e (ratio %.2f), 4 eps32 scale %.2e" % (
            name, mode, k, err, y["e_ref"][k], err / y["e_ref"][k] if y["e_ref"][k] > 0 else float("nan"), 4 * EPS32 * y["scale"][k]))
        assert err <= bound, "%s/%s %s: %.3e > %.3e" % (name, mode, k, err, bound)
        if mode == "nearest" and k in ("g_depth", "g_pose", "g_K"):   # the output does not depend on the position: exact zeros
            assert float(got[k].abs().max()) == 0.0
    if name == "outside_far":     # beyond the [-2, size + 1] clamp: no tap, nothing but zeros
        for k in U.QUANTITIES:
            assert float(got[k].abs().max()) == 0.0, k
        assert not bool(got["valid"].any())


def test_inverse_warp_behind_the_camera(dev):
    """pz < 1e-3: Z is the clamp, whose gradient with respect to pz is zero; X / Z and Y / Z still carry one when a tap is
    inside.  Where no tap is inside g_depth is exactly zero, as float64's; the others are held to the bound of the case."""
    ref = U.inverse_warp_reference("behind", "bilinear")
    got = _hip_cached("behind", "bilinear", dev)
    sel = ref["M"] & (ref["pz"] < 1e-3)
    assert int(sel.sum()) > 50
    none_in = sel & (ref["taps"] == 0)
    assert float(ref["q"]["g_depth"][none_in].abs().max()) == 0.0 and float(got["g_depth"][none_in].abs().max()) == 0.0
    err = U.masked_err(got["g_depth"], ref["q"]["g_depth"], sel)
    assert err <= U.inverse_warp_bound("behind", "bilinear", "g_depth")


@pytest.mark.parametrize("mode", U.MODES)
def test_inverse_warp_many_to_one_scatter_loses_nothing(dev, mode):
    """zoom_many_to_one: 64 atomics per texel (16 in nearest mode).  Two runs agree to 4 eps32 max|g_img| (atomics reorder the
    sum), and per (item, channel) the sum of g_img over the image equals float64's sum of gout * weights to 4 eps32 of it:
    every sample's weights sum to 1 and the upstream gradient is positive, so a lost or overwritten addend is missed whole."""
    c = U.inverse_warp_case("zoom_many_to_one")
    ref = U.inverse_warp_reference("zoom_many_to_one", mode)
    a = _hip_cached("zoom_many_to_one", mode, dev)["g_img"]
    b = _hip(c, mode, dev, ref["gup"])["g_img"]
    scale = float(ref["q"]["g_img"].abs().max())
    assert float((a.double() - b.double()).abs().max()) <= 4 * EPS32 * scale
    want = ref["q"]["g_img"].sum(dim=(2, 3))
    assert bool((want > 0.9 * ref["gup"].double().sum(dim=(2, 3))).all())
    for g in (a, b):
        err = (g.double().sum(dim=(2, 3)) - want).abs()
        print("zoom/%s: sum of g_img off by %.2e of %.2e (bound %.2e)" % (mode, float(err.max()), float(want.max()),
                                                                          4 * EPS32 * float(want.abs().max())))
        assert float(err.max()) <= 4 * EPS32 * float(want.abs().max())


@pytest.mark.parametrize("mode", U.MODES)
def test_inverse_warp_requested_gradient_combinations(dev, mode):
    """The NULL-output paths of pdepth_inverse_warp_backward_f32 (want_img / want_point) against the all-gradients run of
    'ragged': per-pixel results bit for bit, the atomic scatter and the small matrix products to 4 eps32 of their scale."""
    c = U.inverse_warp_case("ragged")
    ref = U.inverse_warp_reference("ragged", mode)
    full = _hip_cached("ragged", mode, dev)
    close = lambda x, y_: float((x.double() - y_.double()).abs().max()) <= 4 * EPS32 * float(y_.abs().max())
    only_img = _hip(c, mode, dev, ref["gup"], need=("img",))                      # grad_point NULL
    assert only_img["g_depth"] is None and only_img["g_pose"] is None and only_img["g_K"] is None
    assert torch.equal(only_img["out"], full["out"]) and close(only_img["g_img"], full["g_img"])
    only_depth = _hip(c, mode, dev, ref["gup"], need=("depth",))                  # grad_img NULL
    assert only_depth["g_img"] is None and torch.equal(only_depth["g_depth"], full["g_depth"])
    cam = _hip(c, mode, dev, ref["gup"], need=("K", "pose"))                      # grad_img NULL, a 4x4 pose
    assert cam["g_img"] is None and cam["g_depth"] is None and c["pose"].shape[1:] == (4, 4)
    if mode == "bilinear":
        assert close(cam["g_pose"], full["g_pose"]) and close(cam["g_K"], full["g_K"])
        assert float(full["g_pose"].abs().max()) > 0 and float(full["g_depth"].abs().max()) > 0
    else:
        assert float(cam["g_pose"].abs().max()) == 0.0 and float(cam["g_K"].abs().max()) == 0.0


@pytest.mark.parametrize("mode", U.MODES)
def test_inverse_warp_non_finite_depth_stays_in_its_pixel(dev, mode):
    """nan_depth: item 0 holds a NaN, a +inf and a -inf depth (the last one gives an infinite, not NaN, position: weights
    inf - inf = NaN while the position compares equal to itself).  The upstream gradient is NOT masked here.
    Item 1 is what it is with finite depths there (per-pixel results and the sums bit for bit, the atomic scatter to 4 eps32
    of its scale).  In item 0 out and g_depth are non-finite at those pixels only and g_img is finite everywhere: a
    non-finite sample has no valid tap.  g_pose and g_K of item 0 are sums over the item's pixels: non-finite in bilinear
    mode (as float64's are: 0 * inf in the chain rule of X / Z), exact zeros in nearest mode; no value is asserted."""
    c = U.inverse_warp_case("nan_depth")
    got = _hip(c, mode, dev, c["gout"])
    clean = _hip(c, mode, dev, c["gout"], depth=c["depth_finite"])
    for k in ("out", "g_depth", "g_pose", "g_K"):
        assert torch.equal(got[k][1], clean[k][1]), k
    assert bool(torch.isfinite(clean["g_img"]).all())
    assert float((got["g_img"][1] - clean["g_img"][1]).abs().max()) <= 4 * EPS32 * float(clean["g_img"][1].abs().max())
    bad = torch.zeros(c["depth"].shape[1:], dtype=torch.bool)
    for (b, y, x, _) in U.NAN_DEPTH_PIXELS:
        assert b == 0
        bad[y, x] = True
    assert bool(torch.isfinite(got["out"][0])[:, ~bad].all()) and bool(torch.isfinite(got["g_depth"][0])[~bad].all())
    assert torch.equal(got["out"][0][:, ~bad], clean["out"][0][:, ~bad])
    assert torch.equal(got["g_depth"][0][~bad], clean["g_depth"][0][~bad])
    assert bool(torch.isfinite(got["g_img"]).all())
    assert float((got["g_img"][0] - clean["g_img"][0]).abs().max()) <= float(c["gout"][0][:, bad].abs().sum()) + 1e-5
    print("nan_depth/%s: item 0 non-finite entries: out %d, g_depth %d, g_pose %d of %d, g_K %d of %d" % (
        mode, int((~torch.isfinite(got["out"][0])).sum()), int((~torch.isfinite(got["g_depth"][0])).sum()),
        int((~torch.isfinite(got["g_pose"][0])).sum()), got["g_pose"][0].numel(),
        int((~torch.isfinite(got["g_K"][0])).sum()), got["g_K"][0].numel()))
