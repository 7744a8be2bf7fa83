"""CPU suite of the SSIM op: the float64 restatement the GPU tests compare against (tests/util_ssim.py) is checked against the
reference's own float32 results (fixture g23_ssim) and against float64 autograd, and the interface against the reference's."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
import util_ssim as U

NAMES = [f"{kind}_md{md}" for md in U.MDS for kind in U.KINDS]


def _t64(c):
    return tuple(torch.from_numpy(c[k]).double() for k in ("x", "y", "g_out"))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(name):
    """max |float64 restatement - the reference's float32 output| <= 4e-6: the float32 reference is at most 2.3e-6 from float64
    over these cases (printed by tests/golden/make_golden_ssim.py)."""
    c = U.cases()[name]
    x, y, _ = _t64(c)
    dist = U.ssim_dist(x, y, c["md"])
    assert tuple(dist.shape) == c["dist"].shape
    err = float((dist - torch.from_numpy(c["dist"]).double()).abs().max())
    print(name, "max |float64 - reference float32| =", err)
    assert err <= 4e-6
    if name.startswith(("same", "const")):
        assert not c["dist"].any()   # the reference's symmetric form: exactly 0 on identical inputs


@pytest.mark.parametrize("name", NAMES)
def test_coefficient_map_gradients_against_autograd(name):
    """The gradient formula of include/pdepth.h in float64 against float64 autograd of the restatement: 1e-10 of the gradient's
    scale, max(|g|, |g_out|) -- on identical inputs the gradient itself is 0 and each of its terms is of the order of g_out."""
    c = U.cases()[name]
    x, y, g = _t64(c)
    x.requires_grad_(True), y.requires_grad_(True)
    (U.ssim_dist(x, y, c["md"]) * g).sum().backward()
    gx, gy = U.ssim_grads(x.detach(), y.detach(), g, c["md"])
    for tag, got, want in (("g_x", gx, x.grad), ("g_y", gy, y.grad)):
        scale = max(float(want.abs().max()), float(g.abs().max()))
        err = float((got - want).abs().max())
        print(name, tag, "max |formula - autograd| =", err, "scale", scale)
        assert err <= 1e-10 * scale


def test_fixture_has_no_window_near_a_clamp_edge():
    """Windows exactly on an edge follow torch.clamp's inclusive rule (the masked cases: two all-zero patches); none lies within
    util_ssim.EDGE of an edge without being on it, so no case of the fixture depends on which side float32 falls."""
    on_edge = {}
    for name, c in U.cases().items():
        x, y, _ = _t64(c)
        raw = U.ssim_parts(x, y, c["md"])["raw"]
        assert not U.near_edge(raw).any(), name
        on_edge[name] = float(((raw == 0) | (raw == 1)).double().mean())
    for md in U.MDS:
        assert on_edge[f"masked_md{md}"] > 0.05 and on_edge[f"same_md{md}"] == 1.0 and on_edge[f"indep_md{md}"] == 0.0


def test_no_cpu_fallback():
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.SSIM(x, x, md=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim(x.clone().requires_grad_(True), x)


def test_reference_signature():
    """losses.loss_blocks.SSIM(x, y, md=1), as losses/loss_blocks.py:47 of the reference; the loss takes the mix as keywords that
    default to the L1 term alone."""
    from pdepth_amd.losses.loss_blocks import SSIM
    params = inspect.signature(SSIM).parameters
    assert list(params) == ["x", "y", "md"] and params["md"].default == 1
    assert all(p.default is inspect.Parameter.empty for p in (params["x"], params["y"]))
    rsc = inspect.signature(lb.rgb_stereo_consistency_loss).parameters
    assert rsc["ssim_weight"].default == 0.0 and rsc["ssim_md"].default == 1
    assert list(rsc)[:6] == ["src_rgb_img", "target_rgb_img", "target_depth_map", "pose_target2src", "intr", "viz"]


def test_entries_refuse_before_any_launch():
    """The C entries check their arguments first (no GPU is touched): null pointers, md outside 1..3, an image smaller than a
    window, more planes than the grid takes."""
    lib = _native.load()
    fwd, bwd = lib.pdepth_ssim_f32, lib.pdepth_ssim_backward_f32
    assert fwd(None, 256, 1, 3, 8, 8, 1, 256, None) == 1 and b"null pointer" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 3, 8, 8, 1, None, None) == 1 and b"null output" in lib.pdepth_last_error()
    assert fwd(256, 256, 0, 3, 8, 8, 1, 256, None) == 1 and b"non-positive" in lib.pdepth_last_error()
    for md in (0, 4, -1):
        assert fwd(256, 256, 1, 3, 8, 8, md, 512, None) == 1 and b"md = 1, 2 or 3" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 3, 4, 9, 2, 512, None) == 1 and b"H=4, W=9" in lib.pdepth_last_error()
    assert fwd(256, 256, 1, 3, 9, 6, 3, 512, None) == 1 and b"at least 7" in lib.pdepth_last_error()
    assert fwd(256, 256, 256, 256, 8, 8, 1, 512, None) == 1 and b"B*C must be at most 65535" in lib.pdepth_last_error()
    assert bwd(256, 256, None, 1, 3, 8, 8, 1, 512, 768, None) == 1 and b"null pointer" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 3, 8, 8, 1, None, None, None) == 1 and b"no gradient requested" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 3, 8, 8, 4, 512, 768, None) == 1 and b"md = 1, 2 or 3" in lib.pdepth_last_error()
    assert bwd(256, 256, 1024, 1, 3, 2, 8, 1, 512, 768, None) == 1 and b"H=2, W=8" in lib.pdepth_last_error()
    assert bwd(256, 512, 1024, 1, 3, 8, 8, 1, 768, 768, None) == 1 and b"alias" in lib.pdepth_last_error()
    assert bwd(256, 512, 1024, 1, 3, 8, 8, 1, 256, None, None) == 1 and b"alias" in lib.pdepth_last_error()


def test_md_outside_the_kernels_is_not_implemented():
    assert _native.SSIM_MD == (1, 2, 3)
    x = torch.rand(1, 3, 12, 12)
    for md in (0, 4):
        with pytest.raises(NotImplementedError, match=f"md={md}"):
            ops.ssim(x, x, md=md)
        with pytest.raises(NotImplementedError, match=f"md={md}"):
            lb.SSIM(x.clone().requires_grad_(True), x, md)
