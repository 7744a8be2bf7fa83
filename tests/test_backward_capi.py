"""CPU suite: the C ABI of the backward passes (pdepth_sweep_backward_f32, pdepth_dpv_reduce_backward_f32,
pdepth_dpv_expect_backward_f32) is exported, keeps ABI 6 and validates its arguments before any launch (no GPU needed: every
call below returns before touching a pointer); the oracle's fp32 autograd matches the reference's gradients (fixture g23)."""
import ctypes

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native
from oracle import ref_cpu as O
from util import golden

NEW = ("pdepth_sweep_backward_f32", "pdepth_dpv_reduce_backward_f32", "pdepth_dpv_expect_backward_f32")
FAKE = 256   # a non-null "device pointer": validation fails before any use of it


def test_new_symbols_exported_abi_unchanged():
    lib = _native.load()
    for sym in NEW:
        assert sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6


def _desc(**kw):
    f = dict(B=1, V=1, C=4, D=8, H=4, W=4, metric=0, algo=0, blas_mode=0, sigma=10.0)
    f.update(kw)
    chw = f["C"] * f["H"] * f["W"]
    return _native.SweepDesc(f["B"], f["V"], f["C"], f["D"], f["H"], f["W"], f["metric"], f["algo"], f["blas_mode"], f["sigma"],
                             chw, f["V"] * chw, chw)


def _cam():
    return _native.Camera(FAKE, FAKE, FAKE, FAKE, FAKE)


def _sweep_bwd(desc, cam, ref=FAKE, src=FAKE, dc=FAKE, gcost=FAKE, gref=FAKE * 2, gsrc=FAKE * 3):
    lib = _native.load()
    rc = lib.pdepth_sweep_backward_f32(ctypes.byref(desc), ctypes.byref(cam), ref, src, dc, gcost, gref, gsrc, None)
    return rc, lib.pdepth_last_error().decode()


def test_sweep_backward_validation():
    rc, msg = _sweep_bwd(_desc(), _cam(), ref=None)
    assert rc == 1 and msg == "pdepth_sweep_backward_f32: null input pointer"
    rc, msg = _sweep_bwd(_desc(), _cam(), gcost=None)
    assert rc == 1 and "null input pointer" in msg
    rc, msg = _sweep_bwd(_desc(), _cam(), gref=None, gsrc=None)
    assert rc == 1 and msg == "pdepth_sweep_backward_f32: no output requested"
    rc, msg = _sweep_bwd(_desc(), _native.Camera(None, FAKE, FAKE, FAKE, FAKE))
    assert rc == 1 and "null camera pointer" in msg
    rc, msg = _sweep_bwd(_desc(B=0), _cam())
    assert rc == 1 and "non-positive dimension" in msg
    rc, msg = _sweep_bwd(_desc(metric=5), _cam())
    assert rc == 1 and "undefined metric" in msg
    rc, msg = _sweep_bwd(_desc(sigma=0.0), _cam())
    assert rc == 1 and "sigma" in msg
    rc, msg = _sweep_bwd(_desc(D=513), _cam())
    assert rc == 1 and "D=513 exceeds" in msg
    rc, msg = _sweep_bwd(_desc(), _cam(), gref=FAKE, gsrc=FAKE)
    assert rc == 1 and "alias" in msg


def test_dpv_backward_validation():
    lib = _native.load()
    rc = lib.pdepth_dpv_reduce_backward_f32(None, FAKE, 1, 4, 2, 2, FAKE, None, None, FAKE * 2, None)
    assert rc == 1 and lib.pdepth_last_error() == b"pdepth_dpv_reduce_backward_f32: null pointer"
    rc = lib.pdepth_dpv_reduce_backward_f32(FAKE, FAKE, 1, 4, 2, 2, None, None, None, FAKE * 2, None)
    assert rc == 1 and b"no incoming gradient" in lib.pdepth_last_error()
    rc = lib.pdepth_dpv_reduce_backward_f32(FAKE, FAKE, 1, 0, 2, 2, FAKE * 3, None, None, FAKE * 2, None)
    assert rc == 1 and b"non-positive dimension" in lib.pdepth_last_error()
    rc = lib.pdepth_dpv_reduce_backward_f32(FAKE, FAKE, 1, 4, 2, 2, FAKE * 3, None, None, FAKE, None)
    assert rc == 1 and b"alias" in lib.pdepth_last_error()
    rc = lib.pdepth_dpv_expect_backward_f32(FAKE, FAKE, 1, 4, 2, 2, 1, None, FAKE * 2, None)
    assert rc == 1 and lib.pdepth_last_error() == b"pdepth_dpv_expect_backward_f32: null pointer"
    rc = lib.pdepth_dpv_expect_backward_f32(FAKE, FAKE, 1, 4, -2, 2, 1, FAKE * 3, FAKE * 2, None)
    assert rc == 1 and b"non-positive dimension" in lib.pdepth_last_error()


def test_bindings_check_plane_counts_before_the_device():
    """D of the gradient / volume against the depth candidates: refused with a message before any device check."""
    ref, src = torch.zeros(1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4)
    cam = [torch.zeros(1, 3, 3), torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 3), torch.zeros(1, 3, 16), torch.zeros(1, 2)]
    with pytest.raises(RuntimeError, match="grad_cost has 6 planes, d_candi has 8 entries"):
        _native.sweep_backward(ref, src, *cam, torch.zeros(8), torch.zeros(1, 6, 4, 4), 10.0)
    with pytest.raises(RuntimeError, match="d_candi has 8 entries, volume has D=6"):
        _native.dpv_reduce_backward(torch.zeros(1, 6, 4, 4), torch.zeros(8), g_depth=torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="d_candi has 8 entries, volume has D=6"):
        _native.dpv_expect_backward(torch.zeros(1, 6, 4, 4), torch.zeros(8), True, torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="no output requested"):
        _native.sweep_backward(ref, src, *cam, torch.zeros(8), torch.zeros(1, 8, 4, 4), 10.0, want_ref=False, want_src=False)


def test_oracle_sweep_backward_matches_reference_fixture():
    """fp32 autograd through the oracle's restatement vs autograd through the reference's est_swp_volume_v4 / log_softmax /
    dpv_to_depthmap (fixture g23)."""
    g = golden("g23_sweep_backward.npz")
    K = torch.from_numpy(g["K"][0])
    R, t, rays = torch.from_numpy(g["R"][0]), torch.from_numpy(g["t"][0]), torch.from_numpy(g["rays"][0])
    cx, cy = g["K"][0, 0, 2], g["K"][0, 1, 2]
    for metric in ("L2", "L1"):
        ref = torch.from_numpy(g["ref"]).requires_grad_(True)
        src = torch.from_numpy(g["src"]).requires_grad_(True)
        cost = O.sweep_cost(ref, src, g["d_candi"], R, t, K, rays, cx, cy, float(g["sigma"]), metric)
        np.testing.assert_allclose(cost.detach().numpy(), g[metric + "_cost"], rtol=1e-5, atol=1e-4)
        (cost * torch.from_numpy(g[metric + "_gcost"])).sum().backward()
        for got, key in ((ref.grad, "_gref"), (src.grad, "_gsrc")):
            want = g[metric + key]
            assert np.abs(got.numpy() - want).max() <= 1e-5 * np.abs(want).max(), metric + key
    for tag, bv_log in (("lsm", True), ("plain", False)):
        x = torch.from_numpy(g[tag + "_in"]).requires_grad_(True)
        depth = O.dpv_to_depthmap(O.log_dpv(x) if bv_log else x, g["d_candi"], BV_log=bv_log)
        (depth * torch.from_numpy(g[tag + "_gdepth"])).sum().backward()
        np.testing.assert_allclose(x.grad.numpy(), g[tag + "_grad"], rtol=1e-5, atol=1e-6 * np.abs(g[tag + "_grad"]).max())
