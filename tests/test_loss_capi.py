"""CPU suite of the training loss: the C ABI of the fused cross-entropy (pdepth_dpv_soft_ce_workspace_bytes, pdepth_dpv_soft_ce_f32,
pdepth_dpv_soft_ce_backward_f32) is declared, bound and exported, keeps ABI 6 and validates its arguments before any launch (no
GPU needed: every call below returns before touching a pointer); losses.get_loss; the torch compositions of utils/ against the
reference's values (fixture g24)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops, synth
from util import golden
import util_loss as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdepth_dpv_soft_ce_workspace_bytes", "pdepth_dpv_soft_ce_f32", "pdepth_dpv_soft_ce_backward_f32")
FAKE = 256   # a non-null, 256-byte aligned "device pointer": validation fails before any use of it
F = ctypes.c_float


def test_new_symbols_declared_bound_exported_abi_unchanged():
    lib = _native.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pdepth.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pdepth_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_native.EXPORTED_SYMBOLS)
    for sym in NEW:
        assert sym in declared and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6


def _fwd(logp=FAKE, dc=FAKE, label=FAKE * 2, depth_gt=None, var=0.3, pw=2.0, mask=None, B=1, D=4, H=2, W=2, loss=FAKE * 3,
         count=FAKE * 4, depth=None, ws=FAKE * 5, ws_bytes=None):
    lib = _native.load()
    if ws_bytes is None:
        ws_bytes = lib.pdepth_dpv_soft_ce_workspace_bytes(max(B, 1), max(H, 1), max(W, 1))
    rc = lib.pdepth_dpv_soft_ce_f32(logp, dc, label, depth_gt, F(var), F(pw), mask, B, D, H, W, loss, count, depth, ws, ws_bytes, None)
    return rc, lib.pdepth_last_error().decode()


def _bwd(logp=FAKE, dc=FAKE, label=FAKE * 2, depth_gt=None, var=0.3, pw=2.0, mask=None, count=FAKE * 3, B=1, D=4, H=2, W=2,
         g_loss=FAKE * 4, g_depth=None, g_logp=FAKE * 5):
    lib = _native.load()
    rc = lib.pdepth_dpv_soft_ce_backward_f32(logp, dc, label, depth_gt, F(var), F(pw), mask, count, B, D, H, W, g_loss, g_depth, g_logp, None)
    return rc, lib.pdepth_last_error().decode()


def test_forward_validation():
    rc, msg = _fwd(logp=None)
    assert rc == 1 and msg == "pdepth_dpv_soft_ce_f32: null pointer"
    rc, msg = _fwd(label=FAKE * 2, depth_gt=FAKE * 6)
    assert rc == 1 and "exactly one label source" in msg
    rc, msg = _fwd(label=None, depth_gt=None)
    assert rc == 1 and "exactly one label source" in msg
    for dims in (dict(B=0), dict(D=0), dict(H=-1), dict(W=0)):
        rc, msg = _fwd(**dims)
        assert rc == 1 and "non-positive dimension" in msg, dims
    for var in (0.0, -1.0, float("nan")):
        rc, msg = _fwd(label=None, depth_gt=FAKE * 6, var=var)
        assert rc == 1 and "variance must be positive" in msg
    rc, msg = _fwd(var=0.0, ws_bytes=0)   # the variance belongs to the from-depth form only: the call gets as far as its workspace
    assert rc == 3 and "workspace" in msg
    rc, msg = _fwd(loss=None)
    assert rc == 1 and "null output pointer" in msg
    lib = _native.load()
    need = lib.pdepth_dpv_soft_ce_workspace_bytes(2, 64, 96)
    assert need >= 2 * (64 * 96 // 256) * 8 and need % 256 == 0
    assert lib.pdepth_dpv_soft_ce_workspace_bytes(0, 64, 96) == 0
    rc, msg = _fwd(B=2, H=64, W=96, ws_bytes=need - 1)
    assert rc == 3 and "workspace" in msg
    rc, msg = _fwd(B=2, H=64, W=96, ws=None, ws_bytes=need)
    assert rc == 3
    rc, msg = _fwd(B=2, H=64, W=96, ws=FAKE + 1, ws_bytes=need)
    assert rc == 3 and "aligned" in msg


def test_backward_validation():
    rc, msg = _bwd(logp=None)
    assert rc == 1 and msg == "pdepth_dpv_soft_ce_backward_f32: null pointer"
    rc, msg = _bwd(label=None)
    assert rc == 1 and "exactly one label source" in msg
    rc, msg = _bwd(label=None, depth_gt=FAKE * 6, var=0.0)
    assert rc == 1 and "variance must be positive" in msg
    rc, msg = _bwd(D=0)
    assert rc == 1 and "non-positive dimension" in msg
    rc, msg = _bwd(count=None)
    assert rc == 1 and "null pointer" in msg
    rc, msg = _bwd(g_loss=None, g_depth=None)
    assert rc == 1 and "no incoming gradient" in msg
    rc, msg = _bwd(g_logp=FAKE)
    assert rc == 1 and "alias" in msg


def test_bindings_refuse_before_the_device():
    x, dc = torch.zeros(1, 6, 4, 4), torch.zeros(6)
    with pytest.raises(RuntimeError, match="d_candi has 8 entries, volume has D=6"):
        _native.dpv_soft_ce(x, torch.zeros(8), label=torch.zeros(1, 6, 4, 4))
    with pytest.raises(RuntimeError, match="exactly one label source"):
        _native.dpv_soft_ce(x, dc)
    with pytest.raises(RuntimeError, match="exactly one label source"):
        _native.dpv_soft_ce(x, dc, label=torch.zeros(1, 6, 4, 4), depth_gt=torch.zeros(1, 4, 4), variance=0.3)
    with pytest.raises(RuntimeError, match="variance > 0"):
        _native.dpv_soft_ce(x, dc, depth_gt=torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match=r"label must be \[1, 6, 4, 4\]"):
        _native.dpv_soft_ce(x, dc, label=torch.zeros(1, 6, 4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dpv_soft_ce(x, [1.0] * 6, label=torch.zeros(1, 6, 4, 4))
    with pytest.raises(RuntimeError, match="no incoming gradient"):
        _native.dpv_soft_ce_backward(x, dc, torch.zeros(1), label=torch.zeros(1, 6, 4, 4))


def test_get_loss():
    from pdepth_amd.losses import get_loss
    from pdepth_amd.losses.losses import BaseLoss, DefaultLoss
    cfg = synth.default_loss_cfg()
    assert cfg.loss.dc_mul == 0.25 and cfg.var.softce == 0.3 and "loss" not in synth.default_cfg()
    loss = get_loss(cfg, 0)
    assert isinstance(loss, BaseLoss) and loss.labels_from_depth is False
    assert isinstance(get_loss(synth.default_loss_cfg(loss_name="default"), 0), DefaultLoss)
    with pytest.raises(NotImplementedError, match="nonesuch"):
        get_loss(synth.default_loss_cfg(loss_name="nonesuch"), 0)
    from pdepth_amd.losses import loss_blocks
    for name in ("soft_cross_entropy_loss", "mean_on_mask", "depth_consistency_loss", "depth_stereo_consistency_loss",
                 "rgb_stereo_consistency_loss", "edge_aware_smoothness_loss"):
        assert callable(getattr(loss_blocks, name))


def test_fixture_inputs_are_the_generators():
    g = golden("g24_loss.npz")
    for k, v in U.checksums(U.make_inputs()).items():
        assert g[k] == v, k
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g24_loss.npz")) <= os.path.getsize(
        os.path.join(REPO, "tests", "golden", "g23_sweep_backward.npz"))


def test_torch_compositions_against_the_reference():
    """gen_soft_label_torch, transform_dmap: to 1 ulp (exp, division and a 4-term product sum: the same torch calls as the
    reference's, the tolerance covers another vector width); minpool and mean_on_mask's inputs: bit for bit."""
    from pdepth_amd.utils import img_utils, inverse_warp
    g = golden("g24_loss.npz")
    inp = U.make_inputs()
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    for s in U.SIDES:
        got = torch.stack(U.soft_labels(inp, img_utils.gen_soft_label_torch, s, "lo")).numpy()
        want = g[f"label_{s}_lo"]
        assert np.array_equal(got == -1, want == -1)
        np.testing.assert_array_max_ulp(got, want, maxulp=1)
    assert (g["label_right_lo"][0, :, 1, 2:5] == -1).all() and not (g["label_left_lo"] == -1).any()
    got = inverse_warp.transform_dmap(t["dmap_left_hi"][0], torch.inverse(t["T_left2right"]), t["K_hi"][0]).numpy()
    assert got.shape == g["transform_dmap"].shape
    np.testing.assert_array_max_ulp(got, g["transform_dmap"], maxulp=1)
    batched = inverse_warp.transform_dmap(t["dmap_left_hi"], torch.inverse(t["T_left2right"]), t["K_hi"])
    np.testing.assert_array_max_ulp(batched[0].numpy(), g["transform_dmap"], maxulp=1)
    d = t["dmap_left_hi"].clone().requires_grad_(True)
    inverse_warp.transform_dmap(d, torch.inverse(t["T_left2right"]), t["K_hi"]).sum().backward()
    assert torch.isfinite(d.grad).all() and float(d.grad.abs().min()) > 0
    assert np.array_equal(img_utils.minpool(t["dmap_left_hi"].unsqueeze(0), 4).numpy(), g["minpool"])
    sparse = t["dmap_left_hi"] * t["mask_left_hi"][:, 0]
    keep = sparse.clone()
    assert np.array_equal(img_utils.minpool(sparse.unsqueeze(0), 4, 1000).numpy(), g["minpool_default"])
    assert torch.equal(sparse, keep)   # (the input is not written)
    assert np.array_equal(img_utils.gaussian_torch(torch.tensor([1.0, 2.0]), torch.tensor(1.5), torch.tensor(0.5)).numpy(),
                          np.exp(-np.float32(0.25) / np.float32(0.5)).astype(np.float32).repeat(2))


def test_torch_loss_blocks_against_the_reference():
    """The terms of losses/loss_blocks.py that need no warp, on CPU tensors, against the reference's values on item 0 of the
    fixture (1e-6 relative: means over a few thousand float32 terms), and their per-item form."""
    from pdepth_amd.losses import loss_blocks as lb
    g = golden("g24_loss.npz")
    t = {k: torch.from_numpy(v) for k, v in U.make_inputs().items()}
    dl = t["dmap_left_hi"][0:1]
    rgb = t["rgb_left"][:, 0]
    got = {"blk_dc": lb.depth_consistency_loss(dl, t["dmap_left_lo"][0:1]),
           "blk_smooth": lb.edge_aware_smoothness_loss([dl.unsqueeze(0)], rgb[0:1], 1),
           "blk_mean_on_mask": lb.mean_on_mask(rgb[0:1], t["mask_left_hi"][0:1])}
    for k, v in got.items():
        assert abs(float(v) - float(g[k])) <= 1e-6 * abs(float(g[k])), (k, float(v), float(g[k]))
    per_item = lb.depth_consistency_loss(t["dmap_left_hi"], t["dmap_left_lo"], per_item=True)
    assert per_item.shape == (U.B,) and abs(float(per_item[0]) - float(g["blk_dc"])) <= 1e-6 * abs(float(g["blk_dc"]))
    K = t["K_hi"].double()
    assert torch.allclose(lb._inv3(K), torch.inverse(K), rtol=1e-12, atol=1e-15)
