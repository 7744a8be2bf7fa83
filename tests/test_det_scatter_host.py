"""CPU suite of the deterministic (order-independent) scattered gradients: the exponent rule pdepth_det_scale_exponent, which the
kernels of csrc/sweep_bwd_det.hip and csrc/scatter_det.hip call as the same inline code, in exact integer / rational arithmetic;
the three new entries refuse bad arguments before any launch (no GPU needed: every call below returns before touching a
pointer); the workspace queries are the header's formula; the ops carry the keyword."""
import ctypes
import inspect
import os
import re
import struct
from fractions import Fraction

import pytest

import pdepth_amd
from pdepth_amd import _native, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 256   # a non-null, 256-byte aligned "device pointer": validation fails before any use of it
NEW = ("pdepth_det_scale_exponent", "pdepth_sweep_backward_det_workspace_bytes", "pdepth_sweep_backward_det_f32",
       "pdepth_loss_dsc_backward_det_workspace_bytes", "pdepth_loss_dsc_backward_det_f32",
       "pdepth_inverse_warp_backward_det_workspace_bytes", "pdepth_inverse_warp_backward_det_f32")


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


DENORM_MIN, FLT_MAX = _f32(1), _f32(0x7f7fffff)
BOUNDS = (DENORM_MIN, _f32(struct.unpack("<I", struct.pack("<f", 1e-30))[0]), 1.0, _f32(struct.unpack("<I", struct.pack("<f", 1e30))[0]), FLT_MAX)


def test_new_symbols_declared_bound_exported_abi_unchanged():
    lib = _native.load()
    for sym in NEW:
        assert sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6
    h = open(os.path.join(REPO, "include", "pdepth.h")).read()
    assert "#define PDEPTH_ABI_VERSION 6" in h
    assert int(eval(re.search(r"#define PDEPTH_DET_EXP_ZERO (.*)", h).group(1))) == _native.DET_EXP_ZERO
    assert int(re.search(r"#define PDEPTH_DET_EXP_NONFINITE (\d+)", h).group(1)) == _native.DET_EXP_NONFINITE


@pytest.mark.parametrize("n", [1, 2 ** 23, 2 ** 31])
@pytest.mark.parametrize("bound", BOUNDS)
def test_scale_exponent_neither_overflows_nor_wastes_bits(bound, n):
    """n 2 bound 2^S <= 2^62 (the int64 cannot overflow) and n bound 2^S > 2^58 (at most 3 bits wasted), exactly."""
    S = _native.load().pdepth_det_scale_exponent(bound, n)
    assert -400 < S < 400, S
    scaled = n * Fraction(bound) * Fraction(2) ** S   # (Fraction(float) is exact)
    print("bound %g n %d: S = %d, n bound 2^S = 2^%.3f" % (bound, n, S, float(__import__("math").log2(scaled))))
    assert 2 * scaled <= 2 ** 62, (bound, n, S)
    assert scaled > 2 ** 58, (bound, n, S)


def test_scale_exponent_sentinels():
    f = _native.load().pdepth_det_scale_exponent
    for n in (1, 2 ** 23, 2 ** 31):
        assert f(0.0, n) == _native.DET_EXP_ZERO and f(-0.0, n) == _native.DET_EXP_ZERO
        for bad in (float("inf"), float("-inf"), float("nan")):
            assert f(bad, n) == _native.DET_EXP_NONFINITE
    assert f(1.0, 0) == _native.DET_EXP_NONFINITE
    assert f(-1.0, 4) == f(1.0, 4)   # a bound is a magnitude
    assert _native.DET_EXP_ZERO == -2 ** 31 and _native.DET_EXP_NONFINITE == 2 ** 31 - 1


def _call(name, *args):
    lib = _native.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.pdepth_last_error().decode()


def _round256(x):
    return (x + 255) // 256 * 256


def test_workspace_queries_are_the_headers_formula():
    lib = _native.load()
    h = open(os.path.join(REPO, "include", "pdepth.h")).read()
    for needed in ("roundup256(16 B) + roundup256(8 B V C H W)", "roundup256(4 B)  + roundup256(8 B H W)",
                   "roundup256(4 B)  + roundup256(8 B C H W)", "17.6 MB at 64 x 128, 281 MB at 256 x 512", "at most two roundings"):
        assert needed in h, needed
    for B, V, C, D, H, W in ((4, 1, 67, 64, 64, 128), (4, 1, 67, 64, 256, 512), (2, 2, 9, 16, 80, 120), (1, 3, 5, 8, 7, 9), (17, 1, 1, 1, 1, 1)):
        desc = _native.SweepDesc(B, V, C, D, H, W, 0, 0, 0, 10.0, C * H * W, V * C * H * W, C * H * W)
        assert lib.pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(desc)) == _round256(16 * B) + _round256(8 * B * V * C * H * W)
        assert lib.pdepth_loss_dsc_backward_det_workspace_bytes(B, H, W) == _round256(4 * B) + _round256(8 * B * H * W)
        assert lib.pdepth_inverse_warp_backward_det_workspace_bytes(B, C, H, W) == _round256(4 * B) + _round256(8 * B * C * H * W)
    desc = _native.SweepDesc(4, 1, 67, 64, 64, 128, 0, 0, 0, 10.0, 0, 0, 0)
    assert round(lib.pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(desc)) / 1e6, 1) == 17.6
    desc = _native.SweepDesc(4, 1, 67, 64, 256, 512, 0, 0, 0, 10.0, 0, 0, 0)
    assert round(lib.pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(desc)) / 1e6) == 281
    # sizes out of range: 0
    bad = _native.SweepDesc(0, 1, 4, 8, 8, 16, 0, 0, 0, 1.0, 0, 0, 0)
    assert lib.pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.pdepth_loss_dsc_backward_det_workspace_bytes(0, 8, 8) == 0 and lib.pdepth_loss_dsc_backward_det_workspace_bytes(1, 4097, 4097) == 0
    assert lib.pdepth_inverse_warp_backward_det_workspace_bytes(1, 0, 8, 8) == 0


def test_argument_validation_of_the_sweep_entry_without_gpu():
    lib = _native.load()
    who = "pdepth_sweep_backward_det_f32"
    B, V, C, D, H, W = 1, 1, 4, 8, 4, 4
    desc = _native.SweepDesc(B, V, C, D, H, W, 0, 1, 0, 10.0, C * H * W, V * C * H * W, C * H * W)
    cam = _native.Camera(*([FAKE] * 5))
    need = lib.pdepth_sweep_backward_det_workspace_bytes(ctypes.byref(desc))

    def call(desc=desc, ref=FAKE, gcost=4 * FAKE, gref=5 * FAKE, gsrc=6 * FAKE, ws=7 * FAKE, ws_bytes=need):
        return _call(who, ctypes.byref(desc), ctypes.byref(cam), ref, 2 * FAKE, 3 * FAKE, gcost, gref, gsrc, ws, ws_bytes, None)

    assert call(ref=None) == (1, f"{who}: null input pointer")
    assert call(gcost=None) == (1, f"{who}: null input pointer")
    assert call(gref=None, gsrc=None) == (1, f"{who}: no output requested")
    rc, msg = call(ws_bytes=need - 1)
    assert rc == 3 and "workspace" in msg and str(need) in msg
    assert call(ws=None)[0] == 3
    rc, msg = call(ws=7 * FAKE + 1)
    assert rc == 3 and "aligned" in msg
    rc, msg = call(gsrc=2 * FAKE)   # grad_src == src
    assert rc == 1 and "alias" in msg
    bad = _native.SweepDesc(B, V, C, D, H, W, 7, 1, 0, 10.0, C * H * W, V * C * H * W, C * H * W)
    rc, msg = call(desc=bad)
    assert rc == 1 and "undefined metric" in msg
    bad = _native.SweepDesc(B, V, C, 513, H, W, 0, 1, 0, 10.0, C * H * W, V * C * H * W, C * H * W)
    assert call(desc=bad)[0] == 1 and "512 planes" in lib.pdepth_last_error().decode()
    bad = _native.SweepDesc(B, V, C, D, H, W, 0, 1, 0, 0.0, C * H * W, V * C * H * W, C * H * W)
    assert call(desc=bad) == (1, f"{who}: sigma must be non-zero")
    bad = _native.SweepDesc(0, V, C, D, H, W, 0, 1, 0, 10.0, C * H * W, V * C * H * W, C * H * W)
    assert call(desc=bad)[0] == 1 and "non-positive" in lib.pdepth_last_error().decode()


def test_argument_validation_of_the_dsc_entry_without_gpu():
    who = "pdepth_loss_dsc_backward_det_f32"
    P = [FAKE * i for i in range(1, 14)]
    need = _native.load().pdepth_loss_dsc_backward_det_workspace_bytes(2, 64, 96)

    def call(B=2, H=64, W=96, src=P[0], g_value=P[8], g_src=P[9], g_tgt=P[10], ws=P[11], ws_bytes=need):
        return _call(who, src, P[1], P[2], P[3], P[4], P[5], 0, P[6], P[7], g_value, B, H, W, g_src, g_tgt, ws, ws_bytes, None)

    assert call(src=None) == (1, f"{who}: null pointer")
    assert call(g_value=None) == (1, f"{who}: null pointer")
    rc, msg = call(g_src=None, g_tgt=None)
    assert rc == 1 and "no gradient requested" in msg
    assert call(B=0) == (1, f"{who}: non-positive dimension")
    rc, msg = call(H=1)
    assert rc == 1 and "at least 2" in msg
    rc, msg = call(H=4097, W=4097)
    assert rc == 1 and "H*W must be at most 2^24" in msg
    rc, msg = call(ws_bytes=need - 1)
    assert rc == 3 and "workspace" in msg
    assert call(ws=None)[0] == 3
    rc, msg = call(ws=P[11] + 1)
    assert rc == 3 and "aligned" in msg


def test_argument_validation_of_the_inverse_warp_entry_without_gpu():
    who = "pdepth_inverse_warp_backward_det_f32"
    P = [FAKE * i for i in range(1, 10)]
    need = _native.load().pdepth_inverse_warp_backward_det_workspace_bytes(2, 3, 32, 48)

    def call(B=2, C=3, H=32, W=48, mode=0, img=P[0], go=P[4], g_img=P[5], g_pt=P[6], ws=P[7], ws_bytes=need):
        return _call(who, img, P[1], P[2], P[3], go, B, C, H, W, mode, g_img, g_pt, ws, ws_bytes, None)

    assert call(img=None) == (1, f"{who}: null pointer")
    assert call(go=None) == (1, f"{who}: null pointer")
    assert call(g_img=None, g_pt=None) == (1, f"{who}: null pointer")
    assert call(H=1) == (1, f"{who}: bad dimension")
    rc, msg = call(mode=7)
    assert rc == 1 and "unknown mode" in msg
    for mode in (0, 1):
        rc, msg = call(mode=mode, ws_bytes=need - 1)
        assert rc == 3 and "workspace" in msg
        assert call(mode=mode, ws=None)[0] == 3
        rc, msg = call(mode=mode, ws=P[7] + 1)
        assert rc == 3 and "aligned" in msg


def test_ops_carry_the_keyword():
    for fn in (ops.sweep_cost, ops.sweep_dpv, ops.depth_stereo_consistency):
        p = inspect.signature(fn).parameters
        assert "deterministic" in p and p["deterministic"].default is None, fn.__name__
        assert list(p)[-1] == "deterministic", fn.__name__   # a new trailing keyword: positional callers are untouched
    for fn in (_native.sweep_backward, _native.inverse_warp_backward, _native.loss_dsc_backward):
        p = inspect.signature(fn).parameters
        assert p["deterministic"].default is False, fn.__name__
    from pdepth_amd.utils import inverse_warp as iv
    assert list(inspect.signature(iv.inverse_warp).parameters) == ["img", "depth", "pose", "intrinsics", "mode", "rotation_mode", "padding_mode"]


def test_the_two_sweep_units_group_planes_alike():
    """Both units run the one body of sweep_bwd_body.hpp: neither has a tile edge, a box cap, sample positions or footprints of
    its own, and the constants tests/util_sweep_backward.py restates the grouping from are the ones of that header."""
    import util_sweep_backward as U
    csrc = os.path.join(REPO, "probabilistic-depth_amd", "csrc")
    body = open(os.path.join(csrc, "sweep_bwd_body.hpp")).read()
    for unit in ("sweep_bwd.hip", "sweep_bwd_det.hip"):
        text = open(os.path.join(csrc, unit)).read()
        code = re.sub(r"//[^\n]*", "", text)   # (the header comments may speak of the helpers)
        assert '#include "sweep_bwd_body.hpp"' in code, unit
        assert re.search(r"sweep_bwd_body\s*<", code), unit
        assert not re.search(r"\b(BT|BTHREADS|BOX_CAP|BCC|\w*TILE\w*)\s*=", code), unit
        assert "plane_sample_pos" not in code and "make_footprint" not in code, unit
        assert "plane_sample_pos(" not in text, unit
    assert os.path.samefile(U.KERNEL, os.path.join(csrc, "sweep_bwd_body.hpp"))
    declared = tuple(int(v) for n in ("BOX_CAP", "BT") for v in re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % n, body))
    assert len(declared) == 2 and declared == U.kernel_constants()   # (each declared exactly once)
    assert "SWEEP_BWD_TILE" not in open(os.path.join(csrc, "kernels.hpp")).read()
