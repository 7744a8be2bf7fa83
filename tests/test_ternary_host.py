"""CPU suite of the ternary census op: the float64 restatement the GPU tests compare against (tests/util_ternary.py) is checked
against the reference's own float32 results (fixture g26_ternary) and its closed-form gradients against float64 autograd; then the
interface against the reference's, and the refusals that are decided before any launch."""
import inspect

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
import util_ternary as U

NAMES = [f"{kind}_md{md}" for md in U.MDS for kind in U.KINDS]


def _t(c, dtype):
    return tuple(torch.from_numpy(c[k]).to(dtype) for k in ("x", "y", "g_out"))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(name):
    """max |float64 restatement - the reference's float32 result|, within the float32 reference's own distance from float64 over
    these cases as tests/golden/make_golden_ternary.py prints it: at most 3.6e-6 for the output (bound 4e-6) and 4.1e-3 for a
    gradient, whose largest element is 10 to 55 (bound 5e-3).  The float32 composition that stands in for the fixture on other
    shapes is the same function in float32: it is held to the same bounds, doubled (two float32 evaluations in different
    summation orders)."""
    c = U.cases()[name]
    md = c["md"]
    x64, y64, g64 = _t(c, torch.float64)
    ref = (U.ternary_dist(x64, y64, md),) + U.ternary_grads(x64, y64, g64, md)
    x32, y32, g32 = _t(c, torch.float32)
    comp = (U.ternary_dist(x32, y32, md),) + U.ternary_grads(x32, y32, g32, md)
    for key, r64, c32 in zip(("dist", "g_x", "g_y"), ref, comp):
        fix = torch.from_numpy(c[key])
        assert tuple(r64.shape) == fix.shape and c32.dtype == torch.float32
        err = float((fix.double() - r64).abs().max())
        err32 = float((c32.double() - r64).abs().max())
        big = float(r64.abs().max())
        print(name, key, "max |float64 - reference float32| = %.3e  |float64 - composition float32| = %.3e  max |f64| = %.3e" % (err, err32, big))
        bound = 4e-6 if key == "dist" else 5e-3
        assert err <= bound
        assert err32 <= 2 * bound


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("same", "const"))])
def test_identical_inputs_are_exactly_zero(name):
    """The reference returns exactly 0 with exactly zero gradients where the two images are equal bit for bit, and so does the
    restatement in both precisions."""
    c = U.cases()[name]
    assert not c["dist"].any() and not c["g_x"].any() and not c["g_y"].any()
    for dtype in (torch.float32, torch.float64):
        x, y, g = _t(c, dtype)
        gx, gy = U.ternary_grads(x, y, g, c["md"])
        assert int(torch.count_nonzero(U.ternary_dist(x, y, c["md"]))) == 0
        assert int(torch.count_nonzero(gx)) == 0 and int(torch.count_nonzero(gy)) == 0


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_gradients_against_autograd(name):
    """The gradient formula of include/pdepth.h (one chain per offset, weight G(p) + G(p+o)) in float64 against float64 autograd of
    the restatement: 1e-10 of the gradient's scale, max(|g|, |g_out|)."""
    c = U.cases()[name]
    x, y, g = _t(c, torch.float64)
    want = U.ternary_grads(x, y, g, c["md"])
    got = U.ternary_grads_analytic(x, y, g, c["md"])
    for tag, a, b in zip(("g_x", "g_y"), got, want):
        scale = max(float(b.abs().max()), float(g.abs().max()))
        err = float((a - b).abs().max())
        print(name, tag, "max |formula - autograd| =", err, "scale", scale)
        assert err <= 1e-10 * scale


def test_the_border_ring_is_zero_and_still_gets_a_gradient():
    c = U.cases()["indep_md2"]
    x, y, g = _t(c, torch.float64)
    dist = U.ternary_dist(x, y, 2)
    ring = 1 - U.inner_mask(dist, 2)
    assert int(torch.count_nonzero(dist * ring)) == 0 and float((dist * (1 - ring)).min()) >= 0 and float(dist.max()) > 0
    assert np.array_equal(c["dist"] * ring.numpy(), np.zeros_like(c["dist"]))
    gx, _ = U.ternary_grads(x, y, g, 2)
    assert float((gx * ring).abs().max()) > 0   # border pixels are neighbours of interior centres


def test_reference_signature_and_import():
    """losses.loss_blocks.TernaryLoss(im, im_warp, max_distance=1), as losses/loss_blocks.py:8 of the reference; the loss takes the
    mix as keywords that default to the L1 term alone."""
    from pdepth_amd.losses.loss_blocks import TernaryLoss
    params = inspect.signature(TernaryLoss).parameters
    assert list(params) == ["im", "im_warp", "max_distance"] and params["max_distance"].default == 1
    assert all(p.default is inspect.Parameter.empty for p in (params["im"], params["im_warp"]))
    rsc = inspect.signature(lb.rgb_stereo_consistency_loss).parameters
    assert rsc["ternary_weight"].default == 0.0 and rsc["ternary_md"].default == 1
    assert rsc["ssim_weight"].default == 0.0 and rsc["ssim_md"].default == 1 and rsc["fused"].default is False
    assert list(rsc)[:6] == ["src_rgb_img", "target_rgb_img", "target_depth_map", "pose_target2src", "intr", "viz"]
    assert list(inspect.signature(ops.ternary).parameters) == ["x", "y", "md"]
    assert list(inspect.signature(_native.ternary_backward).parameters) == ["x", "y", "g_out", "md", "want_x", "want_y"]


def test_binding_refuses_before_any_launch():
    assert _native.TERNARY_MD == (1, 2, 3)
    x = torch.rand(1, 3, 12, 12)
    for md in (0, 4):
        with pytest.raises(NotImplementedError, match=f"md={md}"):
            ops.ternary(x, x, md=md)
        with pytest.raises(NotImplementedError, match=f"md={md}"):
            lb.TernaryLoss(x.clone().requires_grad_(True), x, md)
    with pytest.raises(RuntimeError, match=r"\[B,3,H,W\].*\[1, 2, 12, 12\] and \[1, 2, 12, 12\]"):
        ops.ternary(x[:, :2], x[:, :2])
    with pytest.raises(RuntimeError, match="H=4, W=12.*at least 5"):
        ops.ternary(x[:, :, :4], x[:, :, :4], md=2)
    with pytest.raises(RuntimeError, match="H=12, W=6.*at least 7"):
        _native.ternary_backward(x[..., :6], x[..., :6], torch.zeros(1, 1, 12, 6), 3)
    with pytest.raises(RuntimeError, match=r"one shape, got \[1, 3, 12, 12\] and \[1, 3, 12, 11\]"):
        ops.ternary(x, x[..., :11])
    with pytest.raises(RuntimeError, match="one shape"):
        ops.ternary(x, x[0])
    for call in (lambda: ops.ternary(x, x), lambda: lb.TernaryLoss(x, x, 2), lambda: ops.ternary(x.clone().requires_grad_(True), x),
                 lambda: _native.ternary_backward(x, x, torch.zeros(1, 1, 12, 12))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_entries_refuse_before_any_launch():
    """The C entries check their arguments first (no GPU is touched): null pointers, md outside 1..3, an image smaller than a patch,
    more items than the grid takes, aliased outputs, no gradient asked for."""
    lib = _native.load()
    fwd, bwd = lib.pdepth_ternary_f32, lib.pdepth_ternary_backward_f32
    assert fwd(None, 256, 1, 8, 8, 1, 512, None) == 1 and b"null pointer" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 8, 8, 1, None, None) == 1 and b"null output" in lib.pdepth_last_error()
    assert fwd(256, 256, 0, 8, 8, 1, 512, None) == 1 and b"non-positive" in lib.pdepth_last_error()
    for md in (0, 4, -1):
        assert fwd(256, 256, 1, 8, 8, md, 512, None) == 1 and b"md = 1, 2 or 3" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 4, 9, 2, 512, None) == 1 and b"H=4, W=9" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 9, 6, 3, 512, None) == 1 and b"at least 7" in lib.pdepth_last_error()
    assert fwd(256, 256, 65536, 8, 8, 1, 512, None) == 1 and b"B must be at most 65535" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 1 << 16, 1 << 15, 1, 512, None) == 1 and b"H*W at most 2^30" in lib.pdepth_last_error()
    assert fwd(256, 512, 1, 8, 8, 1, 256, None) == 1 and b"alias" in lib.pdepth_last_error()
    assert bwd(256, 256, None, 1, 8, 8, 1, 512, 768, None) == 1 and b"null pointer" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 8, 8, 1, None, None, None) == 1 and b"no gradient requested" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 8, 8, 4, 512, 768, None) == 1 and b"md = 1, 2 or 3" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 2, 8, 1, 512, 768, None) == 1 and b"H=2, W=8" in lib.pdepth_last_error()
    assert bwd(256, 512, 1024, 1, 8, 8, 1, 768, 768, None) == 1 and b"alias" in lib.pdepth_last_error()
    assert bwd(256, 512, 1024, 1, 8, 8, 1, 256, None, None) == 1 and b"alias" in lib.pdepth_last_error()
    assert bwd(256, 512, 1024, 1, 8, 8, 1, None, 1024, None) == 1 and b"alias" in lib.pdepth_last_error()
    assert lib.pdepth_abi_version() == 6


def test_loss_refuses_the_single_pass_op_with_a_census_term():
    """fused=True is csrc/photo.hip, which has no census term: refused before anything is computed."""
    z = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no census term"):
        lb.rgb_stereo_consistency_loss(z, z, z[:, 0], torch.eye(4)[None], torch.eye(3)[None], fused=True, ternary_weight=0.5)
