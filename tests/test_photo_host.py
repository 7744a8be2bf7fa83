"""CPU suite of the fused photometric term (csrc/photo.hip): the new entries are declared, bound and exported, they check their
arguments before any launch, the binding refuses what it cannot run, and the float64 restatement the GPU suite compares against
(tests/util_photo.py) reduces to the pieces the merged suites pin: util_loss_terms.rsc64 at w = 0, util_ssim.ssim_dist on the
warp's output for its SSIM share.  The maker's assertions are run on every case of the GPU suite."""
import inspect
import os
import re

import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
import util_loss_terms as LT
import util_photo as P
import util_ssim as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdepth_loss_photo_workspace_bytes", "pdepth_loss_photo_f32", "pdepth_loss_photo_backward_f32")


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(REPO, "include", "pdepth.h")).read()
    lib = _native.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    added = header[header.index("backward-compatible additions within 6"):header.index("enum {")]
    assert all(name in added for name in NEW)
    assert lib.pdepth_abi_version() == 6 and "#define PDEPTH_ABI_VERSION 6" in header
    assert "photo.hip" in open(os.path.join(REPO, "probabilistic-depth_amd", "csrc", "Makefile")).read()


def test_workspace_is_twelve_bytes_per_tile_and_item():
    lib = _native.load()
    for B, H, W in ((1, 3, 3), (2, 16, 64), (2, 17, 65), (4, 256, 512), (3, 64, 128)):
        tiles = ((W + 63) // 64) * ((H + 15) // 16)
        assert lib.pdepth_loss_photo_workspace_bytes(B, H, W) == (12 * B * tiles + 255) // 256 * 256
    assert lib.pdepth_loss_photo_workspace_bytes(0, 8, 8) == 0 and lib.pdepth_loss_photo_workspace_bytes(1, 4097, 4096) == 0


def test_entries_refuse_before_any_launch():
    """No GPU is touched: md, sizes, null pointers, a workspace that is missing, short or misaligned (return code 3)."""
    lib = _native.load()
    fwd, bwd, err = lib.pdepth_loss_photo_f32, lib.pdepth_loss_photo_backward_f32, lib.pdepth_last_error
    p = [256, 512, 768, 1024, 1280]   # src_rgb, tgt_rgb, tgt_depth, Kinv, proj: never dereferenced
    need = lib.pdepth_loss_photo_workspace_bytes(2, 17, 65)
    assert need == 256
    ok_tail = (2048, 2304, 4096, need, None)   # value, count, workspace, bytes, stream
    for md in (0, 4, -1):
        assert fwd(*p, 2, 17, 65, 0.85, md, *ok_tail) == 1 and b"md=%d" % md in err() and b"md = 1, 2 or 3" in err()
        assert bwd(*p, 2048, 2304, 2, 17, 65, 0.85, md, 4096, None) == 1 and b"md = 1, 2 or 3" in err()
    assert fwd(*p, 1, 2, 9, 0.85, 1, *ok_tail) == 1 and b"H=2, W=9" in err() and b"at least 3" in err()
    assert fwd(*p, 1, 9, 6, 0.85, 3, *ok_tail) == 1 and b"H=9, W=6" in err() and b"at least 7" in err()
    assert bwd(*p, 2048, 2304, 1, 4, 9, 0.85, 2, 4096, None) == 1 and b"H=4, W=9" in err()
    assert fwd(*p, 0, 17, 65, 0.85, 1, *ok_tail) == 1 and b"non-positive" in err()
    assert fwd(*p, 1, 4097, 4096, 0.85, 1, *ok_tail) == 1 and b"2^24" in err()
    for i in range(5):
        q = list(p)
        q[i] = None
        assert fwd(*q, 2, 17, 65, 0.85, 1, *ok_tail) == 1 and b"null pointer" in err()
        assert bwd(*q, 2048, 2304, 2, 17, 65, 0.85, 1, 4096, None) == 1 and b"null pointer" in err()
    assert fwd(*p, 2, 17, 65, 0.85, 1, None, 2304, 4096, need, None) == 1 and b"null output" in err()
    assert fwd(*p, 2, 17, 65, 0.85, 1, 2048, None, 4096, need, None) == 1 and b"null output" in err()
    assert bwd(*p, None, 2304, 2, 17, 65, 0.85, 1, 4096, None) == 1 and b"null pointer" in err()
    assert bwd(*p, 2048, None, 2, 17, 65, 0.85, 1, 4096, None) == 1 and b"null pointer" in err()
    assert bwd(*p, 2048, 2304, 2, 17, 65, 0.85, 1, None, None) == 1 and b"null pointer" in err()
    assert fwd(*p, 2, 17, 65, 0.85, 1, 2048, 2304, 4096, need - 1, None) == 3 and b"workspace" in err()
    assert fwd(*p, 2, 17, 65, 0.85, 1, 2048, 2304, None, need, None) == 3
    assert fwd(*p, 2, 17, 65, 0.85, 1, 2048, 2304, 4097, need, None) == 3 and b"aligned" in err()


def test_binding_refuses_what_it_cannot_run():
    t = P.make_inputs(1, 7, 7, 1)
    Kinv, proj = (x.float() for x in P.matrices64(t))
    args = (t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgb_stereo_consistency(*args, ssim_weight=0.85)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.loss_photo(*args, 0.85, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lb.rgb_stereo_consistency_loss(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], t["T"][None], t["intr"], ssim_weight=0.85, fused=True)
    with pytest.raises(NotImplementedError, match="md=4"):
        ops.rgb_stereo_consistency(*args, ssim_weight=0.85, ssim_md=4)
    with pytest.raises(RuntimeError, match="H=7, W=6: a window of md=3 needs H and W of at least 7"):
        ops.rgb_stereo_consistency(args[0][..., :6], args[1][..., :6], args[2][..., :6], Kinv, proj, ssim_weight=0.85, ssim_md=3)
    with pytest.raises(RuntimeError, match=r"tgt_rgb must be \[1, 3, 7, 7\]"):
        ops.rgb_stereo_consistency(args[0], args[1][:, :, :6], *args[2:], ssim_weight=0.85)
    with pytest.raises(RuntimeError, match="rgb_stereo_consistency: src_rgb requires grad"):
        ops.rgb_stereo_consistency(args[0].clone().requires_grad_(True), *args[1:], ssim_weight=0.85)
    with pytest.raises(RuntimeError, match="per_item=True"):
        two = P.make_inputs(2, 36, 48, 1)
        lb.rgb_stereo_consistency_loss(two["src_rgb"], two["tgt_rgb"], two["tgt_depth"], two["T"][None], two["intr"], ssim_weight=0.85,
                                       fused=True)


def test_signatures():
    op = inspect.signature(ops.rgb_stereo_consistency).parameters
    assert list(op) == ["src_rgb", "tgt_rgb", "tgt_depth", "Kinv", "proj", "ssim_weight", "ssim_md"]
    assert op["ssim_weight"].default == 0.0 and op["ssim_md"].default == 1
    fn = inspect.signature(lb.rgb_stereo_consistency_loss).parameters
    assert fn["fused"].default is False and list(fn)[-3:] == ["ssim_weight", "ssim_md", "fused"]
    crit = inspect.signature(BaseLoss.__init__).parameters
    assert list(crit) == ["self", "cfg", "id", "labels_from_depth", "fused_terms", "fused_photo"] and crit["fused_photo"].default is False


def _case64(shape, md):
    t = P.make_inputs(*shape, md)
    return t, P.matrices64(t)


@pytest.mark.parametrize("shape", (P.SHAPES[0], P.SHAPES[1], P.SHAPES[-1]))
def test_restatement_without_ssim_is_the_l1_term(shape):
    t, (Kinv, proj) = _case64(shape, 1)
    value, count = P.photo64(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj, 0.0, 1)
    want, want_count = LT.rsc64(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj)
    assert torch.equal(value, want) and torch.equal(count, want_count)


@pytest.mark.parametrize("shape,md", [c for c in P.CASES if c[0] in (P.SHAPES[0], P.SHAPES[1], P.SHAPES[-2])])
def test_restatement_ssim_share_by_hand(shape, md):
    """w = 1: mean(ssim_dist(warped m, tgt m)) / mean(m) from util_loss_terms.warp64 and util_ssim.ssim_dist; w = 0.85: the mix."""
    t, (Kinv, proj) = _case64(shape, md)
    B, H, W = shape
    warped, valid = LT.warp64(t["src_rgb"], t["tgt_depth"], Kinv, proj, "bilinear")
    m = (valid & LT._lower(B, H, W)).double().unsqueeze(1)
    dist = U.ssim_dist(warped * m, t["tgt_rgb"].double() * m, md)
    assert tuple(dist.shape) == (B, 3, H - 2 * md, W - 2 * md)
    share = torch.stack([dist[b].mean() / m[b].mean() for b in range(B)])
    one = P.photo64(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj, 1.0, md)[0]
    assert torch.allclose(one, share, rtol=1e-13, atol=0)
    l1 = LT.rsc64(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj)[0]
    mix = P.photo64(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], Kinv, proj, 0.85, md)[0]
    assert torch.allclose(mix, 0.15 * l1 + 0.85 * share, rtol=1e-13, atol=0)
    assert bool((share > 0).all()) and bool((share < 1).all())


@pytest.mark.parametrize("shape,md", P.CASES)
def test_maker_conditions_hold(shape, md):
    """No window within util_ssim.EDGE of a clamp edge without being on it, every mask non-empty, images in [0, 1], finite
    float64 gradients (make_inputs asserts the first two itself; here on what it returned)."""
    t = P.make_inputs(*shape, md)
    near, least = P.check_inputs(t, md)
    assert near == 0 and least > 0
    for name in ("src_rgb", "tgt_rgb"):
        assert tuple(t[name].shape) == (shape[0], 3) + shape[1:] and float(t[name].min()) >= 0 and float(t[name].max()) <= 1
    Kinv, proj = P.matrices64(t)
    depth = t["tgt_depth"].double().requires_grad_(True)
    value, _ = P.photo64(t["src_rgb"], t["tgt_rgb"], depth, Kinv, proj, P.W_SSIM, md)
    value.sum().backward()
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(depth.grad).all()) and float(depth.grad.abs().max()) > 0
