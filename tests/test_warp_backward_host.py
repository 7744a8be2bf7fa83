"""CPU suite: the C ABI of warp_feature's backward (pdepth_warp_feature_backward_f32, its _det form and the workspace query)
is exported, keeps ABI 6 and validates its arguments before any launch (no GPU needed: every call below returns before touching
a pointer); ops.warp_feature is differentiable on request only; and the yardstick the GPU suite (test_warp_backward_gpu.py)
holds the kernels to is reachable by the reference's own float32 path: the fp32 autograd gradient of the oracle against the
float64 one, within (4 + n) eps32 A on every texel of every case (util_warp_backward.py has the derivation)."""
import ctypes
import inspect

import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops
import util_warps as U
import util_warp_backward as WB

NEW = ("pdepth_warp_feature_backward_f32", "pdepth_warp_feature_backward_det_workspace_bytes", "pdepth_warp_feature_backward_det_f32")
FAKE = 256   # a non-null, 256-byte-aligned "device pointer": validation fails before any use of it


def test_new_symbols_exported_abi_unchanged():
    lib = _native.load()
    for sym in NEW:
        assert sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6


def _desc(**kw):
    f = dict(B=2, V=2, D=8, H=4, W=6, algo=0, blas_mode=0)
    f.update(kw)
    C = f.get("C", f["D"])
    chw = f["D"] * f["H"] * f["W"]
    return _native.SweepDesc(f["B"], f["V"], C, f["D"], f["H"], f["W"], 0, f["algo"], f["blas_mode"], 1.0, 0,
                             f.get("bstride", f["V"] * chw), f.get("vstride", chw))


def _cam():
    return _native.Camera(FAKE, FAKE, FAKE, FAKE, FAKE)


def _formula(B, V, D, H, W):
    up = lambda x: (x + 255) // 256 * 256
    return up(4 * B) + up(8 * B * V * D * H * W)


def _call(det, desc, cam, dc=FAKE, gout=FAKE, gsrc=FAKE * 2, ws=FAKE * 3, ws_bytes=None):
    lib = _native.load()
    d = None if desc is None else ctypes.byref(desc)
    c = None if cam is None else ctypes.byref(cam)
    if det:
        if ws_bytes is None:
            ws_bytes = 1 << 40
        rc = lib.pdepth_warp_feature_backward_det_f32(d, c, dc, gout, gsrc, ws, ws_bytes, None)
    else:
        rc = lib.pdepth_warp_feature_backward_f32(d, c, dc, gout, gsrc, None)
    return rc, lib.pdepth_last_error().decode()


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_validation_before_any_launch(det):
    who = "pdepth_warp_feature_backward_det_f32" if det else "pdepth_warp_feature_backward_f32"
    rc, msg = _call(det, _desc(), _cam(), gout=None)
    assert rc == 1 and msg == f"{who}: null input pointer"
    for kw in ({"dc": None}, {"gsrc": None}):
        rc, msg = _call(det, _desc(), _cam(), **kw)
        assert rc == 1 and "null input pointer" in msg
    rc, msg = _call(det, None, _cam())
    assert rc == 1 and "null descriptor" in msg
    rc, msg = _call(det, _desc(), _native.Camera(FAKE, None, FAKE, FAKE, FAKE))
    assert rc == 1 and msg == f"{who}: null camera pointer"
    for kw in ({"B": 0}, {"V": -1}, {"D": 0, "C": 0}, {"H": 0}, {"W": 0}):
        rc, msg = _call(det, _desc(**kw), _cam())
        assert rc == 1 and "non-positive dimension" in msg, kw
    rc, msg = _call(det, _desc(), _cam(), gout=FAKE, gsrc=FAKE)
    assert rc == 1 and "alias" in msg
    rc, msg = _call(det, _desc(D=513), _cam())
    assert rc == 1 and "D=513 exceeds the 512 planes" in msg
    rc, msg = _call(det, _desc(C=4), _cam())
    assert rc == 1 and "C == D" in msg
    rc, msg = _call(det, _desc(blas_mode=5), _cam())
    assert rc == 1 and "blas_mode" in msg
    rc, msg = _call(det, _desc(vstride=8 * 4 * 6 + 1), _cam())   # grad_src is contiguous: no padded views
    assert rc == 1 and "bad strides" in msg
    rc, msg = _call(det, _desc(B=65536), _cam())
    assert rc == 1 and "65535" in msg


def test_workspace_is_checked_before_any_launch():
    need = _formula(2, 2, 8, 4, 6)
    rc, msg = _call(True, _desc(), _cam(), ws=None, ws_bytes=need)
    assert rc == 3 and "workspace" in msg and "pdepth_warp_feature_backward_det_workspace_bytes" in msg
    rc, msg = _call(True, _desc(), _cam(), ws_bytes=need - 1)
    assert rc == 3 and f"needs {need} bytes" in msg
    rc, msg = _call(True, _desc(), _cam(), ws=FAKE * 3 + 8, ws_bytes=need)
    assert rc == 3 and "aligned" in msg


def test_workspace_query_is_the_formula_of_the_header():
    lib = _native.load()
    q = lambda d: lib.pdepth_warp_feature_backward_det_workspace_bytes(ctypes.byref(d))
    for B, V, D, H, W in ((2, 2, 8, 4, 6), (4, 2, 64, 64, 128), (1, 1, 5, 7, 9), (3, 2, 16, 33, 47), (65, 1, 1, 1, 1)):
        assert q(_desc(B=B, V=V, D=D, H=H, W=W)) == _formula(B, V, D, H, W), (B, V, D, H, W)
    assert _formula(4, 2, 64, 64, 128) == 256 + 8 * 4 * 2 * 64 * 64 * 128
    assert lib.pdepth_warp_feature_backward_det_workspace_bytes(None) == 0
    for kw in ({"B": 0}, {"V": 0}, {"H": -3}, {"W": 0}, {"D": 0, "C": 0}, {"D": 513}, {"C": 4}, {"H": 1 << 16, "W": 1 << 15}):
        assert q(_desc(**kw)) == 0, kw


def test_differentiable_is_opt_in():
    sig = inspect.signature(ops.warp_feature)
    assert sig.parameters["differentiable"].default is False
    assert sig.parameters["deterministic"].default is None
    assert list(sig.parameters)[:8] == ["src", "K", "R", "t", "rays", "cxcy", "d_candi", "blas"]


def test_binding_checks_shapes_before_the_device():
    cam = [torch.zeros(1, 3, 3), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3), torch.zeros(1, 3, 16), torch.zeros(1, 2)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native.warp_feature_backward(torch.zeros(1, 2, 8, 4, 4), *cam, torch.zeros(8))
    dev_less = torch.zeros(1, 2, 8, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_feature(dev_less, *cam, torch.zeros(8), differentiable=True)
    # the plain call refuses a src that requires grad, the differentiable one reaches the device check instead
    with pytest.raises(RuntimeError, match="no backward"):
        ops.warp_feature(dev_less.clone().requires_grad_(True), *cam, torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_feature(dev_less.clone().requires_grad_(True), *cam, torch.zeros(8), differentiable=True)
    with pytest.raises(RuntimeError, match="rays requires grad"):
        cam2 = list(cam)
        cam2[3] = cam[3].clone().requires_grad_(True)
        ops.warp_feature(dev_less.clone().requires_grad_(True), *cam2, torch.zeros(8), differentiable=True)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in U.WARP_FEATURE_CASES])
def test_reference_float32_backward_stays_within_the_bound(name):
    """The fp32 autograd gradient of the reference's own path (O.warp_feature: all D x C planes through F.grid_sample, the
    diagonal kept) against the float64 gradient, on every texel.  Measured with g_out ~ N(0, 1), seed 7: worst error / bound
    between 0.15 and 0.25 over the eleven cases, texels no tap reaches exactly 0; the worst contention is n = 42 taps on a
    texel ('behind')."""
    b = U.warp_feature_case(name)
    ref = WB.reference(name)
    leaf = b["src"].clone().requires_grad_(True)
    out = U.warp_feature_oracle32(b, src=leaf)
    g32, = torch.autograd.grad(out, leaf, ref["g_out"])
    assert g32.dtype == torch.float32
    ratio = WB.check(g32, ref, f"oracle32 backward, {name} (n up to {int(ref['n'].max())})")
    assert ratio > 0.0   # (a float32 sum that matched float64 everywhere would mean the comparison is vacuous)
