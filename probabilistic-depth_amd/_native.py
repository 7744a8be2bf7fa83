"""ctypes binding of the C ABI in include/pdepth.h (libpdepth_hip.so, built in-tree).

The product path has NO CPU fallback: if the shared library is missing or a tensor is not
a contiguous fp32 device tensor, these wrappers raise.  torch is used only for device
memory and the current HIP stream.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpdepth_hip.so")

METRIC_L2, METRIC_L1 = 0, 1
ALGO_AUTO, ALGO_DIRECT, ALGO_TILED_1, ALGO_TILED_2, ALGO_CELLS, ALGO_MFMA, ALGO_CORR, ALGO_DIST = 0, 1, 2, 3, 4, 5, 6, 7
LAYOUT_NONE, LAYOUT_C4, LAYOUT_DIST16 = 0, 1, 3   # (2: a retired layout; pdepth_sweep_source_layout never answers it)
# workspace ints behind the tile flags that the diagnostics below read (csrc/sweep_workspace.hpp; tests/test_capi_symbols.py compares them)
NONCENTRED_SLOT, LAYOUT_SLOT, DIST_DIRECT_LAST_SLOT, DIST_NONCE_SLOT = 51, 56, 59, 60
BLAS_FMA, BLAS_SEPARATE = 0, 1
DET_EXP_ZERO, DET_EXP_NONFINITE = -2 ** 31, 2 ** 31 - 1   # what pdepth_det_scale_exponent answers for a zero / non-finite bound

class SweepDesc(Structure):
    _fields_ = [
        ("B", c_int32), ("V", c_int32), ("C", c_int32), ("D", c_int32), ("H", c_int32), ("W", c_int32),
        ("metric", c_int32), ("algo", c_int32), ("blas_mode", c_int32), ("sigma", c_float),
        ("ref_bstride", c_int64), ("src_bstride", c_int64), ("src_vstride", c_int64),
    ]


class Camera(Structure):
    _fields_ = [("K", c_void_p), ("R", c_void_p), ("t", c_void_p), ("rays", c_void_p), ("cxcy", c_void_p)]


_P, _I, _F, _Z = c_void_p, c_int32, c_float, c_size_t
_DESC, _CAM = POINTER(SweepDesc), POINTER(Camera)
# every entry include/pdepth.h declares: name -> (restype, argtypes).  load() applies it; tests check it against the header
_SIGNATURES = {
    "pdepth_abi_version": (c_int, []),
    "pdepth_last_error": (c_char_p, []),
    "pdepth_sweep_workspace_bytes": (_Z, [_DESC]),
    "pdepth_sweep_source_layout": (c_int, [_DESC]),
    "pdepth_sweep_centres_source": (c_int, [_DESC]),
    "pdepth_sweep_cost_f32": (c_int, [_DESC, _CAM] + [_P] * 5 + [_Z, _P]),
    "pdepth_sweep_dpv_f32": (c_int, [_DESC, _CAM] + [_P] * 7 + [_Z, _P]),
    "pdepth_pack_source_f32": (c_int, [_DESC, _P, _P, _Z, _P]),
    "pdepth_pack_views_f32": (c_int, [_DESC, _P, _P, _I, _P, _P, _Z, _P]),
    "pdepth_sweep_dpv_packed_f32": (c_int, [_DESC, _CAM] + [_P] * 6 + [_Z, _P]),
    "pdepth_sweep_backward_f32": (c_int, [_DESC, _CAM] + [_P] * 7),
    "pdepth_warp_feature_f32": (c_int, [_DESC, _CAM] + [_P] * 4),
    "pdepth_sample_coords_f32": (c_int, [_DESC, _CAM] + [_P] * 4),
    "pdepth_dpv_reduce_f32": (c_int, [_P, _P] + [_I] * 4 + [_P] * 3),
    "pdepth_dpv_reduce_ex_f32": (c_int, [_P] * 3 + [_I] * 4 + [_P] * 6),
    "pdepth_dpv_reduce_backward_f32": (c_int, [_P, _P] + [_I] * 4 + [_P] * 5),
    "pdepth_dpv_reduce_ex_lp": (c_int, [_I] + [_P] * 3 + [_I] * 4 + [_P] * 2 + [_I] + [_P] * 4),
    "pdepth_dpv_reduce_backward_lp": (c_int, [_I, _P, _P] + [_I] * 4 + [_P] * 2 + [_I] + [_P] * 3),
    "pdepth_dpv_expect_f32": (c_int, [_P, _P] + [_I] * 5 + [_P] * 2),
    "pdepth_dpv_expect_backward_f32": (c_int, [_P, _P] + [_I] * 5 + [_P] * 3),
    "pdepth_dpv_moments_f32": (c_int, [_P, _P] + [_I] * 5 + [_P] * 3),
    "pdepth_dpv_fuse_f32": (c_int, [_P] * 4 + [_I] * 4 + [_F, _F] + [_P] * 3),
    "pdepth_dpv_fuse_backward_f32": (c_int, [_P] * 6 + [_I] * 4 + [_F, _F] + [_P] * 2),
    "pdepth_ufield_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_ufield_f32": (c_int, [_P] * 4 + [_I] * 5 + [_F] * 4 + [_I, _F] + [_P] * 3 + [_Z, _P]),
    "pdepth_correlation_output_size": (c_int, [_I] * 7 + [POINTER(c_int32)] * 3),
    "pdepth_correlation_forward_f32": (c_int, [_P] * 2 + [_I] * 10 + [_P] * 2),
    "pdepth_correlation_backward_f32": (c_int, [_P] * 3 + [_I] * 10 + [_P] * 3),
    "pdepth_correlation_forward_f16": (c_int, [_P] * 2 + [_I] * 10 + [_P] * 2),
    "pdepth_correlation_backward_f16": (c_int, [_P] * 3 + [_I] * 10 + [_P] * 3),
    "pdepth_inverse_warp_f32": (c_int, [_P] * 4 + [_I] * 5 + [_P] * 3),
    "pdepth_inverse_warp_backward_f32": (c_int, [_P] * 5 + [_I] * 5 + [_P] * 3),
    "pdepth_dpv_soft_ce_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_dpv_soft_ce_f32": (c_int, [_P] * 4 + [_F, _F, _P] + [_I] * 4 + [_P] * 4 + [_Z, _P]),
    "pdepth_dpv_soft_ce_backward_f32": (c_int, [_P] * 4 + [_F, _F, _P, _P] + [_I] * 4 + [_P] * 4),
    "pdepth_depth_metrics_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_depth_metrics_f32": (c_int, [_P] * 5 + [_F] + [_I] * 4 + [_P] * 4 + [_Z, _P]),
    "pdepth_lidar_depth_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_lidar_depth_f32": (c_int, [_P] * 4 + [_I] * 8 + [_F, _F] + [_P] * 5 + [_Z, _P]),
    "pdepth_loss_terms_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_loss_dsc_f32": (c_int, [_P] * 6 + [_I, _P] + [_I] * 3 + [_P] * 3 + [_Z, _P]),
    "pdepth_loss_dsc_backward_f32": (c_int, [_P] * 6 + [_I] + [_P] * 3 + [_I] * 3 + [_P] * 3),
    "pdepth_loss_rsc_f32": (c_int, [_P] * 5 + [_I] * 3 + [_P] * 3 + [_Z, _P]),
    "pdepth_loss_rsc_backward_f32": (c_int, [_P] * 7 + [_I] * 3 + [_P] * 2),
    "pdepth_loss_dc_f32": (c_int, [_P] * 2 + [_I] * 3 + [_P] * 3 + [_Z, _P]),
    "pdepth_loss_dc_backward_f32": (c_int, [_P] * 4 + [_I] * 3 + [_P] * 3),
    "pdepth_loss_smooth_f32": (c_int, [_P] * 2 + [_I] * 3 + [_P] * 2 + [_Z, _P]),
    "pdepth_loss_smooth_backward_f32": (c_int, [_P] * 3 + [_I] * 3 + [_P] * 2),
    "pdepth_det_scale_exponent": (c_int32, [_F, c_int64]),
    "pdepth_sweep_backward_det_workspace_bytes": (_Z, [_DESC]),
    "pdepth_sweep_backward_det_f32": (c_int, [_DESC, _CAM] + [_P] * 7 + [_Z, _P]),
    "pdepth_loss_dsc_backward_det_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_loss_dsc_backward_det_f32": (c_int, [_P] * 6 + [_I] + [_P] * 3 + [_I] * 3 + [_P] * 3 + [_Z, _P]),
    "pdepth_inverse_warp_backward_det_workspace_bytes": (_Z, [_I] * 4),
    "pdepth_inverse_warp_backward_det_f32": (c_int, [_P] * 5 + [_I] * 5 + [_P] * 3 + [_Z, _P]),
    "pdepth_warp_feature_backward_f32": (c_int, [_DESC, _CAM] + [_P] * 4),
    "pdepth_warp_feature_backward_det_workspace_bytes": (_Z, [_DESC]),
    "pdepth_warp_feature_backward_det_f32": (c_int, [_DESC, _CAM] + [_P] * 4 + [_Z, _P]),
    "pdepth_ssim_f32": (c_int, [_P] * 2 + [_I] * 5 + [_P] * 2),
    "pdepth_ssim_backward_f32": (c_int, [_P] * 3 + [_I] * 5 + [_P] * 3),
    "pdepth_loss_photo_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_loss_photo_f32": (c_int, [_P] * 5 + [_I] * 3 + [c_double, _I] + [_P] * 3 + [_Z, _P]),
    "pdepth_loss_photo_backward_f32": (c_int, [_P] * 7 + [_I] * 3 + [c_double, _I] + [_P] * 2),
    "pdepth_ternary_f32": (c_int, [_P] * 2 + [_I] * 4 + [_P] * 2),
    "pdepth_ternary_backward_f32": (c_int, [_P] * 3 + [_I] * 4 + [_P] * 3),
    "pdepth_range_map_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_range_map_f32": (c_int, [_P] + [_I] * 3 + [_F] + [_P] * 3 + [_Z, _P]),
    "pdepth_depth_range_map_f32": (c_int, [_P] * 4 + [_I] * 3 + [_F] + [_P] * 3 + [_Z, _P]),
    "pdepth_flow_warp_f32": (c_int, [_P] * 2 + [_I] * 5 + [_P] * 2),
    "pdepth_flow_warp_backward_f32": (c_int, [_P] * 3 + [_I] * 5 + [_P] * 3),
    "pdepth_flow_warp_backward_det_workspace_bytes": (_Z, [_I] * 4),
    "pdepth_flow_warp_backward_det_f32": (c_int, [_P] * 3 + [_I] * 5 + [_P] * 3 + [_Z, _P]),
    "pdepth_flow_fb_check_f32": (c_int, [_P] * 2 + [_I] * 3 + [_F] * 2 + [_P] * 2),
    "pdepth_loss_smooth1_f32": (c_int, [_P] * 2 + [_I] * 5 + [_F] + [_P] * 2 + [_Z, _P]),
    "pdepth_loss_smooth1_backward_f32": (c_int, [_P] * 3 + [_I] * 5 + [_F] + [_P] * 2),
    "pdepth_flow_cost_volume_f32": (c_int, [_P] * 3 + [_I] * 5 + [_F, _I] + [_P] * 2),
    "pdepth_flow_cost_volume_backward_workspace_bytes": (_Z, [_I] * 5),
    "pdepth_flow_cost_volume_backward_f32": (c_int, [_P] * 5 + [_I] * 5 + [_F, _I] + [_P] * 4 + [_Z, _P]),
    "pdepth_flow_cost_volume_backward_det_workspace_bytes": (_Z, [_I] * 5),
    "pdepth_flow_cost_volume_backward_det_f32": (c_int, [_P] * 5 + [_I] * 5 + [_F, _I] + [_P] * 4 + [_Z, _P]),
    "pdepth_flow_photo_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_flow_photo_f32": (c_int, [_P] * 4 + [_I] * 4 + [c_double] * 3 + [_P] * 3 + [_Z, _P]),
    "pdepth_flow_photo_backward_f32": (c_int, [_P] * 6 + [_I] * 4 + [c_double] * 3 + [_P] * 2),
    "pdepth_flow_metrics_workspace_bytes": (_Z, [_I] * 3),
    "pdepth_flow_metrics_f32": (c_int, [_P, _I, _P, _I, _I, _P] + [_I] * 3 + [_P] * 4 + [_Z, _P]),
    "pdepth_flow_resize_f32": (c_int, [_P] + [_I] * 6 + [_P] * 2),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
# The entries that live in an object of their own, outside the sweep's: a part of the entry's name -> its source file (the first
# part that matches names it).  The product library must have them all; an experiment library named by PDEPTH_LIB may be linked
# from a subset of the objects: it loads, and a call of such an entry on it raises (_entry)
_SOURCE_OF_ENTRY = {"_loss_photo_": "csrc/photo.hip", "_loss_smooth1_": "csrc/loss_smooth1.hip", "_det_scale_": "csrc/sweep_bwd_det.hip", "_sweep_backward_det_": "csrc/sweep_bwd_det.hip",
                    "_dsc_backward_det_": "csrc/scatter_det.hip", "_inverse_warp_backward_det_": "csrc/scatter_det.hip",
                    "_warp_feature_backward_": "csrc/warp_bwd.hip", "_ssim_": "csrc/ssim.hip", "_ternary_": "csrc/ternary.hip",
                    "_range_map_": "csrc/occlusion.hip", "_flow_cost_volume_": "csrc/cost_volume.hip", "_flow_photo_": "csrc/flow_photo.hip",
                    "_flow_metrics_": "csrc/flow_metrics.hip", "_flow_resize_": "csrc/flow_metrics.hip", "_flow_": "csrc/flow_warp.hip",
                    "_soft_ce_": "csrc/loss.hip", "_depth_metrics_": "csrc/metrics.hip", "_fuse_backward_": "csrc/dpv_fuse_bwd.hip",
                    "_lidar_depth_": "csrc/lidar_depth.hip", "_loss_": "csrc/loss_terms.hip", "_reduce_ex_lp": "csrc/dpv_half.hip",
                    "_reduce_backward_lp": "csrc/dpv_half.hip"}
_ABSENT_FROM_EXPERIMENT_LIBS = tuple(n for n in _SIGNATURES if any(part in n for part in _SOURCE_OF_ENTRY))


_lib = None
_host_blas = None


def host_blas_mode():
    """Which rounding the host BLAS behind torch's CPU matmul uses (include/pdepth.h PDEPTH_BLAS_*).

    The reference's CPU path computes K@R, K@t and (K@R)@rays with torch.matmul (MKL); whether MKL
    fuses multiply-adds depends on the host CPU.  One tiny CPU matmul is compared with both
    closed forms (products/sums evaluated in float64 then rounded, which is exact for one fma)
    so the kernels reproduce the sampling positions of the reference run on THIS host.
    Override with PDEPTH_BLAS_MODE=fma|separate.
    """
    global _host_blas
    if _host_blas is not None:
        return _host_blas
    env = os.environ.get("PDEPTH_BLAS_MODE", "").lower()
    if env in ("fma", "separate"):
        _host_blas = BLAS_FMA if env == "fma" else BLAS_SEPARATE
        return _host_blas
    g = torch.Generator().manual_seed(7)
    A = (torch.randn(3, 3, generator=g) * 100).float()
    Bm = torch.randn(3, 4096, generator=g).float()
    C = A.matmul(Bm).numpy()
    a, b = A.numpy().astype(np.float64), Bm.numpy().astype(np.float64)
    f32 = np.float32
    p = [(a[:, k:k + 1] * b[k:k + 1, :]) for k in range(3)]          # exact products (float64)
    fma = ((p[0].astype(f32).astype(np.float64) + p[1]).astype(f32).astype(np.float64) + p[2]).astype(f32)
    sep = ((p[0].astype(f32) + p[1].astype(f32)).astype(f32) + p[2].astype(f32)).astype(f32)
    bad_fma, bad_sep = int((fma != C).sum()), int((sep != C).sum())
    if bad_fma == 0 or bad_fma < bad_sep:
        _host_blas = BLAS_FMA
    else:
        _host_blas = BLAS_SEPARATE
    return _host_blas


def _no_autograd(who, *tensors):
    """The ctypes kernels are invisible to autograd: refuse inputs that would silently lose (or corrupt) gradients."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(f"{who}: this HIP op has no backward; call it under torch.no_grad() "
                           "(inference only, like the reference's evaluation loop)")


def load():
    """Load libpdepth_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # experiments only (tools/variants_dist.sh): PDEPTH_LIB points at a library built with other kernel knobs
    path = os.environ.get("PDEPTH_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C probabilistic-depth_amd/csrc)")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        if path != LIB_PATH and name in _ABSENT_FROM_EXPERIMENT_LIBS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.pdepth_abi_version() != 6:
        raise RuntimeError("libpdepth_hip.so ABI version mismatch")
    _lib = lib
    return lib


class UnsupportedShape(RuntimeError):
    """The packed entry points do not take this shape: callers use the plain NCHW path instead (every other failure of a
    native call -- launch errors, out of memory -- is a plain RuntimeError and must propagate)."""


def _check(rc, lib):
    if rc != 0:
        msg = lib.pdepth_last_error().decode()
        if rc == 1 and "does not run on a packed source" in msg:   # PDEPTH_E_ARG of the packing entry points for such a shape
            raise UnsupportedShape(msg)
        raise RuntimeError(msg)


def _entry(lib, name):
    """An entry of the loaded library that lives in an object of its own (_SOURCE_OF_ENTRY); a library linked without that
    object is an error here, there is no other path."""
    fn = getattr(lib, name, None)
    if fn is None:
        source = next(src for part, src in _SOURCE_OF_ENTRY.items() if part in name)
        raise RuntimeError(f"{name}: the loaded library was linked without {source}; there is no fallback")
    return fn


def _volume_dims(who, volume, d_candi, name):
    """(B, D, H, W) of a [B,D,H,W] volume (`name` in the message) with one depth candidate per plane."""
    if volume.dim() != 4:
        raise RuntimeError(f"{who}: {name} must be [B,D,H,W]")
    D = volume.shape[1]
    if d_candi.numel() != D:
        raise RuntimeError(f"{who}: d_candi has {d_candi.numel()} entries, volume has D={D}")
    return tuple(volume.shape)


def _refuse(t, name, dtype=None, device=True):
    """Raise what is wrong with tensor argument `name`: the three refusals of a tensor, stated here and nowhere else, tried in this
    order -- not a tensor; not on the device (unless device=False: judged later); not of `dtype` (if one is given).  Callers test the
    conditions inline, so a well-formed call pays for no message and no frame."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if device and not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a device tensor (got {t.device}); there is no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {str(dtype).replace('torch.', '')}, got {t.dtype}")


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> int:
    """data_ptr() of one device tensor of `dtype` (contiguity is the caller's business)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        _refuse(t, name, dtype)
    return t.data_ptr()


def _tensors(who, fp32="cast", **named):
    """The contiguous device tensors an entry takes, in the order given (shapes are the caller's business).  who: the prefix of the
    message, or None for the bare name.  fp32 = "cast": the device is judged tensor by tensor, then each is widened to fp32 (a loss
    term reads a mask or a half map as fp32); "insist": every tensor must be fp32 already, judged for all of them before any device
    (a position in half precision is another position); None: the dtypes are the caller's business."""
    if fp32 == "insist":
        for name, t in named.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                _refuse(t, f"{who}: {name}" if who else name, torch.float32, device=False)
    out = []
    for name, t in named.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            _refuse(t, f"{who}: {name}" if who else name)
        out.append(t.float().contiguous() if fp32 == "cast" else t.contiguous())
    return out


def _optional(**named):
    """_tensors (bare names, cast to fp32) over arguments that may be None: None stays None."""
    return [t if t is None else _tensors(None, **{name: t})[0] for name, t in named.items()]


def _ptr(t):
    return None if t is None else t.data_ptr()


# the element types of the half-precision reductions (pdepth_dpv_reduce_ex_lp): torch dtype -> PDEPTH_DTYPE_*
DTYPE_F16, DTYPE_BF16 = 1, 2
_LP_DTYPES = {torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev) -> int:
    """hipStream_t of torch's current stream on `dev` (the raw getter where this torch has it: the Stream object costs 4 us)."""
    if _raw_stream is not None and dev.index is not None:
        return _raw_stream(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


_DEVICE_IS_CURRENT = contextlib.nullcontext()


def _on_device(dev):
    """torch.cuda.device(dev) only when another device is current (the context manager costs more than a small sweep's launch)."""
    return _DEVICE_IS_CURRENT if dev.index is None or torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _call(name, dev, *args):
    """C entry `name` on torch's current stream of `dev`: resolved through _entry, the device made current only if it is not, the
    stream appended as the last argument, the return code checked."""
    lib = _lib if _lib is not None else load()
    with _on_device(dev):
        rc = _entry(lib, name)(*args, _stream(dev))
    _check(rc, lib)


def _ask(name, *args):
    """What a C entry that takes no stream answers: a workspace size, a layout, an exponent."""
    return _entry(_lib if _lib is not None else load(), name)(*args)


def _workspace(nbytes, dev):
    """(tensor | None, nbytes) of an entry's workspace: None at zero bytes, which the size queries answer only for sizes the entry
    refuses before it looks at its workspace."""
    return (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes) if nbytes else (None, 0)


_desc_cache = {}   # (B, V, C, D, H, W, metric, algo) -> (workspace bytes, staging layout): two library calls saved per sweep


def _workspace_and_layout(desc):
    key = (desc.B, desc.V, desc.C, desc.D, desc.H, desc.W, desc.metric, desc.algo)
    hit = _desc_cache.get(key)
    if hit is None:
        hit = (_ask("pdepth_sweep_workspace_bytes", ctypes.byref(desc)), _ask("pdepth_sweep_source_layout", ctypes.byref(desc)))
        if len(_desc_cache) < 4096:
            _desc_cache[key] = hit
    return hit


def _inner_contiguous(t: torch.Tensor, n_inner: int) -> bool:
    """True if the last n_inner dims are laid out densely (row-major)."""
    exp = 1
    for size, stride in zip(reversed(t.shape[-n_inner:]), reversed(t.stride()[-n_inner:])):
        if size != 1 and stride != exp:
            return False
        exp *= size
    return True


def _camera(K, R, t, rays, cxcy, B, V, HW):
    for nm, x, shape in (("K", K, (B, 3, 3)), ("R", R, (B, V, 3, 3)), ("t", t, (B, V, 3)),
                         ("rays", rays, (B, 3, HW)), ("cxcy", cxcy, (B, 2))):
        if tuple(x.shape) != shape:
            raise RuntimeError(f"{nm}: expected shape {shape}, got {tuple(x.shape)}")
    K, R, t, rays, cxcy = (x.contiguous() for x in (K, R, t, rays, cxcy))
    cam = Camera(_dev(K, "K"), _dev(R, "R"), _dev(t, "t"), _dev(rays, "rays"), _dev(cxcy, "cxcy"))
    return cam, (K, R, t, rays, cxcy)  # keep the contiguous copies alive


def _blas(blas_mode):
    return host_blas_mode() if blas_mode is None else int(blas_mode)


def selected_kernel(B, V, C, D, H, W, metric=METRIC_L2, algo=ALGO_AUTO):
    """Name of the sweep kernel family a descriptor selects ('dist' | 'tiled' | 'direct'): pdepth_sweep_source_layout."""
    desc = SweepDesc(B, V, C, D, H, W, int(metric), int(algo), BLAS_FMA, 1.0, C * H * W, V * C * H * W, C * H * W)
    return {LAYOUT_DIST16: "dist", LAYOUT_C4: "tiled"}.get(_ask("pdepth_sweep_source_layout", ctypes.byref(desc)), "direct")


class PackedSource:
    """Source views [B,V,C,H,W] in the sweep kernels' staging layout (pdepth_pack_source_f32): a workspace to hand to
    sweep() in place of src, for callers that sweep the same source features more than once or write them once per
    frame.  Owns its device memory; do not use it from two streams at once."""

    def __init__(self, ws, shape, layout=LAYOUT_C4):
        self.ws, self.shape = ws, tuple(shape)   # shape = (B, V, C, H, W)
        self.layout = int(layout)                # LAYOUT_* : the kernel family it was packed for (pdepth_sweep_source_layout)

    @property
    def centred(self):
        """The channel means were subtracted (pdepth_sweep_centres_source)."""
        return self.layout == LAYOUT_DIST16


def pack_source(src, n_planes=64, algo=ALGO_AUTO, metric=METRIC_L2):
    """src [B,V,C,H,W] fp32 device tensor -> PackedSource (n_planes and algo only select the kernel that will sweep it, like
    desc.D and desc.algo: the layout the distance-form kernel takes is mean-centred, the LDS-tiled kernel's is not)."""
    _no_autograd("pack_source", src)
    _dev(src, "src")
    if src.dim() != 5:
        raise RuntimeError("pack_source: src must be [B,V,C,H,W]")
    B, V, C, H, W = src.shape
    if not _inner_contiguous(src, 3) or (V > 1 and src.stride(1) < C * H * W):
        src = src.contiguous()
    desc = SweepDesc(B, V, C, int(n_planes), H, W, int(metric), int(algo), BLAS_FMA, 1.0, C * H * W,
                     src.stride(0) if B > 1 else V * C * H * W, src.stride(1) if V > 1 else C * H * W)
    ws, ws_bytes = _workspace(_ask("pdepth_sweep_workspace_bytes", ctypes.byref(desc)), src.device)
    _call("pdepth_pack_source_f32", src.device, ctypes.byref(desc), src.data_ptr(), _ptr(ws), ws_bytes)
    return PackedSource(ws, (B, V, C, H, W), _ask("pdepth_sweep_source_layout", ctypes.byref(desc)))


def pack_views(feat, rgb, n_views, n_planes=64):
    """The encoder epilogue in one pass (pdepth_pack_views_f32): feat [B*V1, Cf, h, w] (encoder output, view V1-1 of every
    item = the reference view), rgb [B*V1, 3, H, W] -> (PackedSource of the V1-1 source views with Cf+3 channels -- the
    pooled image appended like models/models.py:518-520 --, reference-view features [B, Cf+3, h, w]).  Raises for shapes
    the packed sweep does not take (callers fall back to cat + sweep)."""
    _no_autograd("pack_views", feat, rgb)
    _dev(feat, "feat"), _dev(rgb, "rgb")
    if feat.dim() != 4 or rgb.dim() != 4 or feat.shape[0] != rgb.shape[0] or rgb.shape[1] != 3 or feat.shape[0] % n_views:
        raise RuntimeError("pack_views: feat [B*V1,Cf,h,w] and rgb [B*V1,3,H,W] expected")
    feat, rgb = feat.contiguous(), rgb.contiguous()
    N, Cf, h, w = feat.shape
    rate = rgb.shape[3] // w if w else 0
    if rate < 1 or rgb.shape[2] != h * rate or rgb.shape[3] != w * rate or n_views < 2:
        raise UnsupportedShape("pack_views: the image must be an exact integral multiple of the feature map "
                               "(got image %dx%d for a %dx%d map), with at least one source view"
                               % (rgb.shape[2], rgb.shape[3], h, w))
    B, V, C = N // n_views, n_views - 1, Cf + 3
    desc = SweepDesc(B, V, C, int(n_planes), h, w, METRIC_L2, ALGO_AUTO, BLAS_FMA, 1.0, C * h * w, V * C * h * w, C * h * w)
    ws, ws_bytes = _workspace(_ask("pdepth_sweep_workspace_bytes", ctypes.byref(desc)), feat.device)
    ref = torch.empty((B, C, h, w), dtype=torch.float32, device=feat.device)
    _call("pdepth_pack_views_f32", feat.device, ctypes.byref(desc), feat.data_ptr(), rgb.data_ptr(), rate, ref.data_ptr(), _ptr(ws), ws_bytes)
    return PackedSource(ws, (B, V, C, h, w), _ask("pdepth_sweep_source_layout", ctypes.byref(desc))), ref


def sweep(ref, src, K, R, t, rays, cxcy, d_candi, sigma, metric=METRIC_L2, algo=ALGO_AUTO,
          want_cost=True, want_logp=False, want_depth=False, blas_mode=None):
    """Batched plane sweep (+ optional fused DPV reduction).

    ref [B,C,H,W], src [B,V,C,H,W] (batch/view strides free, inner C,H,W dense) or a PackedSource, K [B,3,3],
    R [B,V,3,3], t [B,V,3], rays [B,3,HW], cxcy [B,2], d_candi [D] -- fp32 device tensors.
    Returns (cost | None, logp | None, depth | None).
    """
    packed = src if isinstance(src, PackedSource) else None
    _no_autograd("sweep", ref, None if packed else src)
    _dev(ref, "ref")
    if ref.dim() != 4:
        raise RuntimeError("sweep: ref must be [B,C,H,W] and src [B,V,C,H,W]")
    B, C, H, W = ref.shape
    if packed:
        if (packed.shape[0], packed.shape[2], packed.shape[3], packed.shape[4]) != (B, C, H, W):
            raise RuntimeError(f"sweep: packed source {packed.shape} does not match ref {tuple(ref.shape)}")
        if packed.ws.device != ref.device:
            raise RuntimeError("sweep: packed source lives on another device")
        V = packed.shape[1]
    else:
        _dev(src, "src")
        if src.dim() != 5:
            raise RuntimeError("sweep: ref must be [B,C,H,W] and src [B,V,C,H,W]")
        V = src.shape[1]
        if tuple(src.shape) != (B, V, C, H, W):
            raise RuntimeError(f"sweep: src shape {tuple(src.shape)} does not match ref {tuple(ref.shape)}")
        if not _inner_contiguous(src, 3) or (V > 1 and src.stride(1) < C * H * W) or (B > 1 and src.stride(0) < 0):
            src = src.contiguous()   # (e.g. an expanded view: view stride 0)
    if not _inner_contiguous(ref, 3):
        ref = ref.contiguous()
    d_candi = d_candi.contiguous()
    D = d_candi.numel()
    dev = ref.device
    cam, keep = _camera(K, R, t, rays, cxcy, B, V, H * W)
    desc = SweepDesc(B, V, C, D, H, W, int(metric), int(algo), _blas(blas_mode), float(sigma),
                     ref.stride(0) if B > 1 else C * H * W,
                     (src.stride(0) if B > 1 else V * C * H * W) if not packed else V * C * H * W,
                     (src.stride(1) if V > 1 else C * H * W) if not packed else C * H * W)
    ws_bytes, layout = _workspace_and_layout(desc)
    if packed:
        if ws_bytes == 0 or packed.ws.numel() < ws_bytes:
            raise RuntimeError("sweep: this shape / algorithm does not run on a packed source")
        if layout != packed.layout:
            raise RuntimeError("sweep: the source was packed for another kernel family (layout %d, centred: %s); pack it with "
                               "the algo / n_planes / metric it will be swept with" % (packed.layout, packed.centred))
        ws = packed.ws
    else:
        ws, ws_bytes = _workspace(ws_bytes, dev)
    cost = torch.empty((B, D, H, W), dtype=torch.float32, device=dev) if want_cost else None
    logp = torch.empty((B, D, H, W), dtype=torch.float32, device=dev) if want_logp else None
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    inputs = (ref.data_ptr(),) if packed else (ref.data_ptr(), src.data_ptr())   # (the packed entry reads the source from the workspace)
    _call("pdepth_sweep_dpv_packed_f32" if packed else "pdepth_sweep_dpv_f32", dev, ctypes.byref(desc), ctypes.byref(cam), *inputs,
          _dev(d_candi, "d_candi"), _ptr(cost), _ptr(logp), _ptr(depth), _ptr(ws), ws_bytes)
    del keep
    global _last_workspace
    _last_workspace = ws  # diagnostics only: tile flags of the last sweep (see fallback_tiles())
    return cost, logp, depth


_last_workspace = None


def _tiles_and_queue_offset(B, H, W):
    """(tile flags of a workspace, byte offset of the 64 queue ints behind them): csrc/sweep_workspace.hpp."""
    n = B * ((W + 15) // 16) * ((H + 3) // 4)
    return n, (4 * n + 255) & ~255


def _queue_slot(B, H, W, slot):
    at = _tiles_and_queue_offset(B, H, W)[1] + 4 * slot
    return int(_last_workspace[at: at + 4].view(torch.int32).item())


def noncentred_guard(B, H, W):
    """Diagnostics: did the pre-pass of the last sweep on a NOT centred source (LDS-tiled kernel) find channel offsets larger
    than the spread of the features -- the tiled kernel then evaluated every plane directly (csrc/sweep_workspace.hpp)."""
    return None if _last_workspace is None else _queue_slot(B, H, W, NONCENTRED_SLOT) != 0


def fallback_tiles(B, H, W, gather_flag=1):
    """Diagnostics: how much of the last sweep left the fast path.  After the distance-form kernel (ALGO_AUTO / 'dist' on its
    shapes): passes over a block of 16 pixels it evaluated directly (the kernel zeroes its count per call); after the
    LDS-tiled kernel: 16x4 tiles left to the gather kernel.  gather_flag: the tile-flag value counted (the gather kernel's
    is 1)."""
    if _last_workspace is None:
        return 0
    n = _tiles_and_queue_offset(B, H, W)[0]
    direct = 0
    if _queue_slot(B, H, W, LAYOUT_SLOT) == LAYOUT_DIST16:   # (nonce << 20) | count; a count tagged by another call's nonce is stale (sweep_workspace.hpp: DIST_NONCE_SLOT)
        tagged, nonce = _queue_slot(B, H, W, DIST_DIRECT_LAST_SLOT), _queue_slot(B, H, W, DIST_NONCE_SLOT)
        direct = (tagged & 0xFFFFF) if nonce != 0 and (tagged >> 20) == nonce else 0
    return int((_last_workspace[: 4 * n].view(torch.int32) == gather_flag).sum().item()) + direct


def dpv_reduce(logits, d_candi, want_logp=True, want_depth=True, inplace=False):
    """logits [B,D,H,W] -> (logp [B,D,H,W] | None, depth [B,H,W] | None)."""
    _no_autograd("dpv_reduce", logits)   # (in place it would also overwrite a tensor that carries a grad_fn)
    if isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in _LP_DTYPES:
        out = dpv_reduce_ex(logits, d_candi, None, want_logp, False, want_depth)   # (fp32 outputs: nothing to write in place)
        return out.get("logp"), out.get("depth")
    _dev(logits, "logits")
    B, D, H, W = _volume_dims("dpv_reduce", logits, d_candi, "logits")
    logits, d_candi = logits.contiguous(), d_candi.contiguous()
    dev = logits.device
    logp = (logits if inplace else torch.empty_like(logits)) if want_logp else None
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    _call("pdepth_dpv_reduce_f32", dev, logits.data_ptr(), _dev(d_candi, "d_candi"), B, D, H, W, _ptr(logp), _ptr(depth))
    return logp, depth


def _reduce_ex_out(B, D, H, W, dev, logp, prob, want_depth, want_var, want_quarter):
    """dict of the requested outputs of a dpv_reduce_ex call.  logp and prob are the caller's, a tensor or None (their dtype, and
    whether logp is the input itself, differ between the fp32 and the half entry); the others are fp32 and made here."""
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"logp": logp, "prob": prob, "depth": f32(B, H, W) if want_depth else None, "var": f32(B, H, W) if want_var else None,
           "quarter": f32(B, D, H // 4, W // 4) if want_quarter else None}
    return {k: v for k, v in out.items() if v is not None}


def _dpv_reduce_ex_lp(logits, d_candi, addend, want_logp, want_prob, want_depth, want_var, want_quarter, prob_dtype):
    """dpv_reduce_ex on fp16 / bf16 logits (pdepth_dpv_reduce_ex_lp): every output fp32, prob in prob_dtype."""
    who, dtype = "dpv_reduce_ex", logits.dtype
    if addend is not None and logits.dim() == 4:
        if isinstance(addend, torch.Tensor) and addend.dtype != dtype:
            raise RuntimeError(f"{who}: addend is {addend.dtype}, logits are {dtype}: both must be of one dtype "
                               "(cast the fp32 one down, or the half one up with .float())")
        _dev(addend, "addend", dtype)
        if addend.shape != logits.shape:
            raise RuntimeError(f"{who}: addend shape {tuple(addend.shape)} != logits {tuple(logits.shape)}")
        addend = addend.contiguous()
    if prob_dtype not in (None, torch.float32, dtype):
        raise RuntimeError(f"{who}: prob_dtype must be torch.float32 or the logits' {dtype}, got {prob_dtype}")
    prob_lp = prob_dtype == dtype
    B, D, H, W = _volume_dims(who, logits, d_candi, "logits")
    logits, d_candi = logits.contiguous(), d_candi.contiguous()
    dev = logits.device
    f32 = lambda: torch.empty((B, D, H, W), dtype=torch.float32, device=dev)
    out = _reduce_ex_out(B, D, H, W, dev, f32() if want_logp else None,
                         (torch.empty_like(logits) if prob_lp else f32()) if want_prob else None, want_depth, want_var, want_quarter)
    _call("pdepth_dpv_reduce_ex_lp", dev, _LP_DTYPES[dtype], logits.data_ptr(), _ptr(addend), _dev(d_candi, "d_candi"), B, D, H, W,
          _ptr(out.get("logp")), _ptr(out.get("prob")), int(prob_lp), _ptr(out.get("depth")), _ptr(out.get("var")), _ptr(out.get("quarter")))
    return out


def dpv_reduce_ex(logits, d_candi, addend=None, want_logp=True, want_prob=False, want_depth=False, want_var=False,
                  want_quarter=False, inplace=False, prob_dtype=None):
    """(logits [+ addend]) [B,D,H,W] -> dict of the requested outputs: logp, prob = exp(logp) [B,D,H,W], depth, var
    [B,H,W], quarter = nearest quarter-resolution logp [B,D,H//4,W//4] -- one pass (pdepth_dpv_reduce_ex_f32).
    fp16 / bf16 logits (and addend, of the same dtype) are widened in the load (pdepth_dpv_reduce_ex_lp): the outputs are
    fp32, prob is fp32 or, with prob_dtype=logits.dtype, of that dtype; inplace is ignored there, the output being another type."""
    _no_autograd("dpv_reduce_ex", logits, addend)
    if isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype in _LP_DTYPES:
        return _dpv_reduce_ex_lp(logits, d_candi, addend, want_logp, want_prob, want_depth, want_var, want_quarter, prob_dtype)
    _dev(logits, "logits")
    if prob_dtype not in (None, torch.float32):
        raise RuntimeError(f"dpv_reduce_ex: prob_dtype must be torch.float32 or the logits' {logits.dtype}, got {prob_dtype}")
    if isinstance(addend, torch.Tensor) and addend.dtype != logits.dtype and addend.dtype in _LP_DTYPES:
        raise RuntimeError(f"dpv_reduce_ex: addend is {addend.dtype}, logits are {logits.dtype}: both must be of one dtype "
                           "(cast the fp32 one down, or the half one up with .float())")
    if addend is not None and logits.dim() == 4:   # (the addend's shape before the candidates: the order these checks have had)
        _dev(addend, "addend")
        if addend.shape != logits.shape:
            raise RuntimeError(f"dpv_reduce_ex: addend shape {tuple(addend.shape)} != logits {tuple(logits.shape)}")
        addend = addend.contiguous()
    B, D, H, W = _volume_dims("dpv_reduce_ex", logits, d_candi, "logits")
    logits, d_candi = logits.contiguous(), d_candi.contiguous()
    dev = logits.device
    out = _reduce_ex_out(B, D, H, W, dev, (logits if inplace else torch.empty_like(logits)) if want_logp else None,
                         torch.empty_like(logits) if want_prob else None, want_depth, want_var, want_quarter)
    _call("pdepth_dpv_reduce_ex_f32", dev, logits.data_ptr(), _ptr(addend), _dev(d_candi, "d_candi"), B, D, H, W,
          _ptr(out.get("logp")), _ptr(out.get("prob")), _ptr(out.get("depth")), _ptr(out.get("var")), _ptr(out.get("quarter")))
    return out


def ufield(dpv, d_candi, intr, mask, bv_log, unc_ang, z_start, z_end, min_depth, quash, d_sum=None):
    """dpv [B,D,H,W], intr [B,3,3], mask [B,H,W] | None -> (plane [B,D,W], depth_zero [B,H,W])  (pdepth_ufield_f32)."""
    _no_autograd("ufield", dpv)
    _dev(dpv, "dpv"), _dev(intr, "intr")
    if dpv.dim() != 4:
        raise RuntimeError("ufield: dpv must be [B,D,H,W]")
    dpv = dpv.contiguous()
    B, D, H, W = dpv.shape
    intr = intr.contiguous().float()
    if tuple(intr.shape) != (B, 3, 3):
        raise RuntimeError(f"ufield: intr must be [{B},3,3], got {tuple(intr.shape)}")
    if mask is not None:
        _dev(mask, "mask")
        if tuple(mask.shape) != (B, H, W):
            raise RuntimeError(f"ufield: mask must be [{B},{H},{W}], got {tuple(mask.shape)}")
        mask = mask.contiguous().float()
    d_candi = d_candi.contiguous()
    # depth of rows shifted in from outside the image: dpv_to_depthmap of the zero padding (exp(0) = 1 per plane).  d_sum = that
    # sum formed by the caller on the host (ops.ufield); a caller that only has the candidates on the device pays one read-back.
    oob = (float(d_sum) if d_sum is not None else float(d_candi.sum().item())) if bv_log else 0.0
    dev = dpv.device
    ws, ws_bytes = _workspace(_ask("pdepth_ufield_workspace_bytes", B, H, W), dev)
    plane = torch.empty((B, D, W), dtype=torch.float32, device=dev)
    dzero = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _call("pdepth_ufield_f32", dev, dpv.data_ptr(), _dev(d_candi, "d_candi"), intr.data_ptr(), _ptr(mask), B, D, H, W, 1 if bv_log else 0,
          float(unc_ang), float(np.float32(z_start)), float(np.float32(z_end)), float(min_depth), 1 if quash else 0, oob,
          plane.data_ptr(), dzero.data_ptr(), _ptr(ws), ws_bytes)
    return plane, dzero


def dpv_expect(dpv, d_candi, bv_log):
    """dpv [B,D,H,W] -> depth [B,H,W] = sum_k d_k * (exp(dpv) if bv_log else dpv)."""
    _no_autograd("dpv_expect", dpv)
    _dev(dpv, "dpv")
    B, D, H, W = _volume_dims("dpv_expect", dpv, d_candi, "dpv")
    dpv, d_candi = dpv.contiguous(), d_candi.contiguous()
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dpv.device)
    _call("pdepth_dpv_expect_f32", dpv.device, dpv.data_ptr(), _dev(d_candi, "d_candi"), B, D, H, W, int(bool(bv_log)), depth.data_ptr())
    return depth


def dpv_moments(dpv, d_candi, bv_log=True):
    """dpv [B,D,H,W] -> (mean [B,H,W], variance [B,H,W]) of the depth distribution."""
    _no_autograd("dpv_moments", dpv)
    _dev(dpv, "dpv")
    B, D, H, W = _volume_dims("dpv_moments", dpv, d_candi, "dpv")
    dpv, d_candi = dpv.contiguous(), d_candi.contiguous()
    mean = torch.empty((B, H, W), dtype=torch.float32, device=dpv.device)
    var = torch.empty_like(mean)
    _call("pdepth_dpv_moments_f32", dpv.device, dpv.data_ptr(), _dev(d_candi, "d_candi"), B, D, H, W, int(bool(bv_log)),
          mean.data_ptr(), var.data_ptr())
    return mean, var


def warp_feature(src, K, R, t, rays, cxcy, d_candi, blas_mode=None):
    """src [B,V,D,H,W] -> out [B,V,D,H,W], channel i warped with depth plane i."""
    _no_autograd("warp_feature", src)
    _dev(src, "src")
    if src.dim() != 5:
        raise RuntimeError("warp_feature: src must be [B,V,D,H,W]")
    B, V, C, H, W = src.shape
    if not _inner_contiguous(src, 3) or (V > 1 and src.stride(1) < C * H * W) or (B > 1 and src.stride(0) < 0):
        src = src.contiguous()   # (e.g. an expanded view: view stride 0)
    d_candi = d_candi.contiguous()
    D = d_candi.numel()
    cam, keep = _camera(K, R, t, rays, cxcy, B, V, H * W)
    desc = SweepDesc(B, V, C, D, H, W, 0, 0, _blas(blas_mode), 1.0, 0, src.stride(0) if B > 1 else V * C * H * W,
                     src.stride(1) if V > 1 else C * H * W)
    out = torch.empty((B, V, D, H, W), dtype=torch.float32, device=src.device)
    _call("pdepth_warp_feature_f32", src.device, ctypes.byref(desc), ctypes.byref(cam), src.data_ptr(), _dev(d_candi, "d_candi"), out.data_ptr())
    del keep
    return out


def warp_feature_backward(g_out, K, R, t, rays, cxcy, d_candi, blas_mode=None, deterministic=False):
    """g_out [B,V,D,H,W] -> g_src [B,V,D,H,W], the gradient of warp_feature with respect to src (the forward is linear in src:
    nothing of it is needed): pdepth_warp_feature_backward_f32, summed with float atomics (last bits depend on the order of
    arrival) unless deterministic: pdepth_warp_feature_backward_det_f32 sums it as 64-bit integers in a workspace of 8 bytes per
    element, allocated here -- the same bits from call to call (a non-finite g_out makes that item's g_src NaN throughout:
    include/pdepth.h)."""
    who = "warp_feature_backward"
    _dev(g_out, "g_out")
    if g_out.dim() != 5:
        raise RuntimeError(f"{who}: g_out must be [B,V,D,H,W]")
    B, V, D, H, W = g_out.shape
    if d_candi.numel() != D:
        raise RuntimeError(f"{who}: d_candi has {d_candi.numel()} entries, g_out has D={D}")
    g_out, d_candi = g_out.contiguous(), d_candi.contiguous()
    cam, keep = _camera(K, R, t, rays, cxcy, B, V, H * W)
    desc = SweepDesc(B, V, D, D, H, W, 0, 0, _blas(blas_mode), 1.0, 0, V * D * H * W, D * H * W)   # (algo 0: as warp_feature)
    g_src = torch.empty_like(g_out)
    dev = g_out.device
    args = (ctypes.byref(desc), ctypes.byref(cam), _dev(d_candi, "d_candi"), g_out.data_ptr(), g_src.data_ptr())
    if deterministic:
        ws, ws_bytes = _workspace(_ask("pdepth_warp_feature_backward_det_workspace_bytes", ctypes.byref(desc)), dev)
        _call("pdepth_warp_feature_backward_det_f32", dev, *args, _ptr(ws), ws_bytes)
    else:
        _call("pdepth_warp_feature_backward_f32", dev, *args)
    del keep
    return g_src


def sample_coords(K, R, t, rays, cxcy, d_candi, H, W, blas_mode=None, algo=ALGO_AUTO):
    """Diagnostic: (ix, iy) [B,V,D,H,W] sample positions handed to the bilinear sampler.

    algo selects the arithmetic of the sweep kernel of the same name: ALGO_AUTO = the shared-reciprocal divide
    chain of the LDS-tiled kernel, ALGO_DIRECT = the compiler's IEEE divides of the gather kernel."""
    _dev(K, "K")
    B, V = R.shape[0], R.shape[1]
    d_candi = d_candi.contiguous()
    D = d_candi.numel()
    cam, keep = _camera(K, R, t, rays, cxcy, B, V, H * W)
    desc = SweepDesc(B, V, 1, D, H, W, 0, int(algo), _blas(blas_mode), 1.0, 0, 0, H * W)
    ix = torch.empty((B, V, D, H, W), dtype=torch.float32, device=K.device)
    iy = torch.empty_like(ix)
    _call("pdepth_sample_coords_f32", K.device, ctypes.byref(desc), ctypes.byref(cam), _dev(d_candi, "d_candi"), ix.data_ptr(), iy.data_ptr())
    del keep
    return ix, iy


def dpv_fuse(logp, dmaps, masks, d_candi, var, eps, want_fused=True, want_log=True):
    """logp [B,D,H,W], dmaps [B,H,W], masks [B,H,W] -> (fused | None, log fused | None)."""
    _no_autograd("dpv_fuse", logp)
    _dev(logp, "logp")
    logp, dmaps, masks, d_candi = (t.contiguous() for t in (logp, dmaps, masks, d_candi))
    B, D, H, W = logp.shape
    if tuple(dmaps.shape) != (B, H, W) or tuple(masks.shape) != (B, H, W) or d_candi.numel() != D:
        raise RuntimeError("dpv_fuse: dmaps/masks must be [B,H,W] and d_candi [D]")
    fused = torch.empty_like(logp) if want_fused else None
    logf = torch.empty_like(logp) if want_log else None
    _call("pdepth_dpv_fuse_f32", logp.device, logp.data_ptr(), _dev(dmaps, "dmaps"), _dev(masks, "masks"), _dev(d_candi, "d_candi"),
          B, D, H, W, float(var), float(eps), _ptr(fused), _ptr(logf))
    return fused, logf


def _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2):
    oc, oh, ow = c_int32(), c_int32(), c_int32()
    rc = _ask("pdepth_correlation_output_size", H, W, int(pad_size), int(kernel_size), int(max_displacement), int(stride1), int(stride2),
              ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow))
    _check(rc, load())
    return oc.value, oh.value, ow.value


def _corr_dtype(x1, x2):
    if x1.dtype != x2.dtype or x1.dtype not in (torch.float32, torch.float16):
        raise RuntimeError("correlation: inputs must both be float32 or both float16 (got %s, %s)" % (x1.dtype, x2.dtype))
    return x1.dtype == torch.float16


def _dev_any(t, name):
    """Device + contiguity check for tensors that may be fp16 (the fp32-only _dev() guards everything else)."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("%s must be a CUDA/HIP tensor (the HIP path has no CPU fallback)" % name)
    if torch.is_grad_enabled() and t.requires_grad:
        raise RuntimeError("%s requires grad: the HIP kernels are invisible to autograd (use ops.correlation / torch.no_grad())" % name)
    return t


def correlation_forward(x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply=1):
    """x1, x2 [B,C,H,W] fp32 or fp16 -> [B,(2*(d/s2)+1)^2,oH,oW] of the same dtype (mean over the kernel window and C of
    shifted products; every configuration of the reference's kernel: include/pdepth.h)."""
    _dev_any(x1, "input1"), _dev_any(x2, "input2")
    if x1.shape != x2.shape or x1.dim() != 4:
        raise RuntimeError("correlation: inputs must be two [B,C,H,W] tensors of the same shape")
    half = _corr_dtype(x1, x2)
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    out = torch.empty((B, oc, oh, ow), dtype=x1.dtype, device=x1.device)
    _call("pdepth_correlation_forward_f16" if half else "pdepth_correlation_forward_f32", x1.device, x1.data_ptr(), x2.data_ptr(), B, C, H, W,
          int(pad_size), int(kernel_size), int(max_displacement), int(stride1), int(stride2), int(corr_multiply), out.data_ptr())
    return out


def correlation_backward(x1, x2, grad_out, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply=1,
                         want1=True, want2=True):
    """x1, x2 [B,C,H,W], grad_out [B,(2r+1)^2,oH,oW] (fp32 or fp16, all alike) -> (grad_x1 | None, grad_x2 | None)."""
    _dev_any(x1, "input1"), _dev_any(x2, "input2"), _dev_any(grad_out, "grad_output")
    half = _corr_dtype(x1, x2)
    x1, x2, grad_out = x1.contiguous(), x2.contiguous(), grad_out.contiguous().to(x1.dtype)
    B, C, H, W = x1.shape
    oc, oh, ow = _corr_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if x2.shape != x1.shape or tuple(grad_out.shape) != (B, oc, oh, ow):
        raise RuntimeError("correlation_backward: shape mismatch")
    g1 = torch.empty_like(x1) if want1 else None
    g2 = torch.empty_like(x2) if want2 else None
    _call("pdepth_correlation_backward_f16" if half else "pdepth_correlation_backward_f32", x1.device, x1.data_ptr(), x2.data_ptr(),
          grad_out.data_ptr(), B, C, H, W, int(pad_size), int(kernel_size), int(max_displacement), int(stride1), int(stride2),
          int(corr_multiply), _ptr(g1), _ptr(g2))
    return g1, g2


SAMPLE_MODES = {"bilinear": 0, "nearest": 1}


def inverse_warp(img, depth, Kinv, proj, mode="bilinear"):
    """img [B,C,H,W], depth [B,H,W], Kinv [B,3,3], proj [B,3,4] -> (warped [B,C,H,W], valid bool [B,H,W])."""
    _dev(img, "img")
    img, depth, Kinv, proj = (t.contiguous() for t in (img, depth, Kinv, proj))
    B, C, H, W = img.shape
    if tuple(depth.shape) != (B, H, W) or tuple(Kinv.shape) != (B, 3, 3) or tuple(proj.shape) != (B, 3, 4):
        raise RuntimeError("inverse_warp: expected depth [B,H,W], Kinv [B,3,3], proj [B,3,4]")
    out = torch.empty_like(img)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=img.device)
    _call("pdepth_inverse_warp_f32", img.device, img.data_ptr(), _dev(depth, "depth"), _dev(Kinv, "Kinv"), _dev(proj, "proj"),
          B, C, H, W, SAMPLE_MODES[mode], out.data_ptr(), valid.data_ptr())
    return out, valid.bool()


def inverse_warp_backward(img, depth, Kinv, proj, grad_out, mode="bilinear", want_img=True, want_point=True, deterministic=False):
    """-> (grad_img [B,C,H,W] | None, grad_point [B,3,H,W] | None): pdepth_inverse_warp_backward_f32; deterministic:
    pdepth_inverse_warp_backward_det_f32 (grad_img as an order-independent sum; grad_point has the same bits either way)."""
    img, depth, Kinv, proj, grad_out = (t.contiguous() for t in (img, depth, Kinv, proj, grad_out))
    B, C, H, W = img.shape
    if tuple(grad_out.shape) != (B, C, H, W):
        raise RuntimeError("inverse_warp_backward: grad_out must have the shape of img")
    g_img = torch.empty_like(img) if want_img else None
    g_pt = torch.empty((B, 3, H, W), dtype=torch.float32, device=img.device) if want_point else None
    args = (_dev(img, "img"), _dev(depth, "depth"), _dev(Kinv, "Kinv"), _dev(proj, "proj"), _dev(grad_out, "grad_out"), B, C, H, W,
            SAMPLE_MODES[mode], _ptr(g_img), _ptr(g_pt))
    if deterministic:
        ws, ws_bytes = _workspace(_ask("pdepth_inverse_warp_backward_det_workspace_bytes", B, C, H, W) if want_img else 0, img.device)
        _call("pdepth_inverse_warp_backward_det_f32", img.device, *args, _ptr(ws), ws_bytes)
    else:
        _call("pdepth_inverse_warp_backward_f32", img.device, *args)
    return g_img, g_pt


# ---- backward passes (ops.py wraps them in torch.autograd.Function) --------------------------------------------------------
def _shape(t, shape, name, who):
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{who}: {name} must be {list(shape)}, got {list(t.shape)}")


def sweep_backward(ref, src, K, R, t, rays, cxcy, d_candi, grad_cost, sigma, metric=METRIC_L2, want_ref=True, want_src=True,
                   blas_mode=None, deterministic=False):
    """grad_cost [B,D,H,W] -> (grad_ref [B,C,H,W] | None, grad_src [B,V,C,H,W] | None): pdepth_sweep_backward_f32.
    ref / src / camera as sweep() (NCHW source only).  grad_ref is reproducible bit for bit; grad_src is summed with float
    atomics (last bits depend on the order of arrival) unless deterministic: pdepth_sweep_backward_det_f32 sums it as 64-bit
    integers in a workspace of 8 bytes per element, allocated here -- the same bits from call to call (a non-finite input makes
    that item's grad_src NaN throughout: include/pdepth.h)."""
    who = "sweep_backward"
    if not (want_ref or want_src):
        raise RuntimeError(f"{who}: no output requested")
    if ref.dim() != 4 or src.dim() != 5:
        raise RuntimeError(f"{who}: ref must be [B,C,H,W] and src [B,V,C,H,W]")
    B, C, H, W = ref.shape
    V = src.shape[1]
    _shape(src, (B, V, C, H, W), "src", who)
    D = d_candi.numel()
    if grad_cost.dim() != 4 or grad_cost.shape[1] != D:
        raise RuntimeError(f"{who}: grad_cost has {grad_cost.shape[1] if grad_cost.dim() == 4 else '?'} planes, d_candi has {D} entries")
    _shape(grad_cost, (B, D, H, W), "grad_cost", who)
    _dev(ref, "ref"), _dev(src, "src"), _dev(grad_cost, "grad_cost"), _dev(d_candi, "d_candi")
    ref, src, d_candi, grad_cost = ref.contiguous(), src.contiguous(), d_candi.contiguous(), grad_cost.contiguous()
    cam, keep = _camera(K, R, t, rays, cxcy, B, V, H * W)
    desc = SweepDesc(B, V, C, D, H, W, int(metric), ALGO_DIRECT, _blas(blas_mode), float(sigma), C * H * W, V * C * H * W, C * H * W)
    g_ref = torch.empty_like(ref) if want_ref else None
    g_src = torch.empty_like(src) if want_src else None
    dev = ref.device
    args = (ctypes.byref(desc), ctypes.byref(cam), ref.data_ptr(), src.data_ptr(), d_candi.data_ptr(), grad_cost.data_ptr(),
            _ptr(g_ref), _ptr(g_src))
    if deterministic:
        ws, ws_bytes = _workspace(_ask("pdepth_sweep_backward_det_workspace_bytes", ctypes.byref(desc)) if want_src else 0, dev)
        _call("pdepth_sweep_backward_det_f32", dev, *args, _ptr(ws), ws_bytes)
    else:
        _call("pdepth_sweep_backward_f32", dev, *args)
    del keep
    return g_ref, g_src


def _grad(g, name, keep=None):
    """An optional incoming gradient: None, or the contiguous fp32 device tensor of it (left in dtype `keep` if it comes in that)."""
    if g is None:
        return None
    dtype = keep if g.dtype == keep else torch.float32
    g = g.contiguous().to(dtype)
    _dev(g, name, dtype)
    return g


def _reduce_backward_args(who, logp, d_candi, g_logp, g_prob, g_depth):
    """((B, D, H, W), logp, d_candi) of the two dpv_reduce backwards: some gradient comes in, each has the shape of its output (judged
    where the tensors live), logp and d_candi are fp32 device tensors."""
    if g_logp is None and g_prob is None and g_depth is None:
        raise RuntimeError(f"{who}: no incoming gradient")
    B, D, H, W = _volume_dims(who, logp, d_candi, "logp")
    for nm, g, shp in (("g_logp", g_logp, (B, D, H, W)), ("g_prob", g_prob, (B, D, H, W)), ("g_depth", g_depth, (B, H, W))):
        if g is not None:
            _shape(g, shp, nm, who)
    _dev(logp, "logp"), _dev(d_candi, "d_candi")
    return (B, D, H, W), logp.contiguous(), d_candi.contiguous()


def dpv_reduce_backward(logp, d_candi, g_logp=None, g_prob=None, g_depth=None):
    """Saved logp [B,D,H,W] + any of g_logp, g_prob [B,D,H,W], g_depth [B,H,W] -> g_logits [B,D,H,W]
    (pdepth_dpv_reduce_backward_f32)."""
    (B, D, H, W), logp, d_candi = _reduce_backward_args("dpv_reduce_backward", logp, d_candi, g_logp, g_prob, g_depth)
    g_logp, g_prob, g_depth = _grad(g_logp, "g_logp"), _grad(g_prob, "g_prob"), _grad(g_depth, "g_depth")
    out = torch.empty_like(logp)
    _call("pdepth_dpv_reduce_backward_f32", logp.device, logp.data_ptr(), d_candi.data_ptr(), B, D, H, W, _ptr(g_logp), _ptr(g_prob),
          _ptr(g_depth), out.data_ptr())
    return out


def dpv_reduce_backward_lp(logp, d_candi, dtype, g_logp=None, g_prob=None, g_depth=None):
    """dpv_reduce_backward with g_logits in `dtype` (torch.float16 | torch.bfloat16), the fp32 value rounded once; g_prob is read
    in fp32 or in `dtype`, as it comes: no copy of either (pdepth_dpv_reduce_backward_lp)."""
    who = "dpv_reduce_backward_lp"
    if dtype not in _LP_DTYPES:
        raise RuntimeError(f"{who}: dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    (B, D, H, W), logp, d_candi = _reduce_backward_args(who, logp, d_candi, g_logp, g_prob, g_depth)
    g_logp, g_depth, g_prob = _grad(g_logp, "g_logp"), _grad(g_depth, "g_depth"), _grad(g_prob, "g_prob", keep=dtype)
    prob_lp = g_prob is not None and g_prob.dtype == dtype
    out = torch.empty(logp.shape, dtype=dtype, device=logp.device)
    _call("pdepth_dpv_reduce_backward_lp", logp.device, _LP_DTYPES[dtype], logp.data_ptr(), d_candi.data_ptr(), B, D, H, W, _ptr(g_logp),
          _ptr(g_prob), int(prob_lp), _ptr(g_depth), out.data_ptr())
    return out


def dpv_expect_backward(dpv, d_candi, bv_log, g_depth):
    """dpv [B,D,H,W], g_depth [B,H,W] -> g_dpv [B,D,H,W] (pdepth_dpv_expect_backward_f32)."""
    who = "dpv_expect_backward"
    B, D, H, W = _volume_dims(who, dpv, d_candi, "dpv")
    _shape(g_depth, (B, H, W), "g_depth", who)
    _dev(dpv, "dpv"), _dev(d_candi, "d_candi")
    dpv, d_candi, g_depth = dpv.contiguous(), d_candi.contiguous(), _grad(g_depth, "g_depth")
    out = torch.empty_like(dpv)
    _call("pdepth_dpv_expect_backward_f32", dpv.device, dpv.data_ptr(), d_candi.data_ptr(), B, D, H, W, int(bool(bv_log)),
          g_depth.data_ptr(), out.data_ptr())
    return out


def dpv_fuse_backward(logp, dmaps, masks, d_candi, var, eps, g_fused=None, g_logfused=None):
    """The inputs of dpv_fuse + any of g_fused, g_logfused [B,D,H,W] -> g_logp [B,D,H,W] (pdepth_dpv_fuse_backward_f32)."""
    who = "dpv_fuse_backward"
    if g_fused is None and g_logfused is None:
        raise RuntimeError(f"{who}: no incoming gradient")
    if logp.dim() != 4:
        raise RuntimeError(f"{who}: logp must be [B,D,H,W]")
    B, D, H, W = logp.shape
    if tuple(dmaps.shape) != (B, H, W) or tuple(masks.shape) != (B, H, W) or d_candi.numel() != D:
        raise RuntimeError(f"{who}: dmaps/masks must be [B,H,W] and d_candi [D]")
    for nm, g in (("g_fused", g_fused), ("g_logfused", g_logfused)):
        if g is not None:
            _shape(g, (B, D, H, W), nm, who)
    _dev(logp, "logp"), _dev(dmaps, "dmaps"), _dev(masks, "masks"), _dev(d_candi, "d_candi")
    logp, dmaps, masks, d_candi = (t.contiguous() for t in (logp, dmaps, masks, d_candi))
    g_fused, g_logfused = _grad(g_fused, "g_fused"), _grad(g_logfused, "g_logfused")
    out = torch.empty_like(logp)
    _call("pdepth_dpv_fuse_backward_f32", logp.device, logp.data_ptr(), dmaps.data_ptr(), masks.data_ptr(), d_candi.data_ptr(),
          _ptr(g_fused), _ptr(g_logfused), B, D, H, W, float(var), float(eps), out.data_ptr())
    return out


# ---- training loss (ops.dpv_soft_ce) ------------------------------------------------------------------------------------------
def _soft_ce_args(who, logp, d_candi, label, depth_gt, variance, mask, pow):
    """Shape checks (before any device check) and the contiguous fp32 tensors of the two cross-entropy entries."""
    B, D, H, W = _volume_dims(who, logp, d_candi, "logp")
    if (label is None) == (depth_gt is None):
        raise RuntimeError(f"{who}: give exactly one label source, label [B,D,H,W] or depth_gt [B,H,W]")
    if label is not None:
        _shape(label, (B, D, H, W), "label", who)
    else:
        _shape(depth_gt, (B, H, W), "depth_gt", who)
        if variance is None or not float(variance) > 0.0:
            raise RuntimeError(f"{who}: the from-depth form needs variance > 0")
    if mask is not None:
        _shape(mask, (B, H, W), "mask", who)
    _dev(logp, "logp"), _dev(d_candi, "d_candi")
    label, depth_gt, mask = _optional(label=label, depth_gt=depth_gt, mask=mask)
    var = float(variance) if depth_gt is not None else 0.0
    return (B, D, H, W), logp.contiguous(), d_candi.contiguous(), label, depth_gt, mask, var, float(pow)


def dpv_soft_ce(logp, d_candi, label=None, depth_gt=None, variance=None, mask=None, want_depth=False, pow=2.0):
    """logp [B,D,H,W] + (label [B,D,H,W] | depth_gt [B,H,W], variance) [+ mask [B,H,W]] -> (loss [B], count [B], depth [B,H,W] |
    None): pdepth_dpv_soft_ce_f32 on the current stream, no host synchronisation."""
    who = "dpv_soft_ce"
    _no_autograd(who, logp)
    (B, D, H, W), logp, d_candi, label, depth_gt, mask, var, pw = _soft_ce_args(who, logp, d_candi, label, depth_gt, variance, mask, pow)
    dev = logp.device
    out = torch.empty((2, B), dtype=torch.float32, device=dev)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    ws, ws_bytes = _workspace(_ask("pdepth_dpv_soft_ce_workspace_bytes", B, H, W), dev)
    _call("pdepth_dpv_soft_ce_f32", dev, logp.data_ptr(), d_candi.data_ptr(), _ptr(label), _ptr(depth_gt), var, pw, _ptr(mask), B, D, H, W,
          out[0].data_ptr(), out[1].data_ptr(), _ptr(depth), _ptr(ws), ws_bytes)
    return out[0], out[1], depth


def dpv_soft_ce_backward(logp, d_candi, count, label=None, depth_gt=None, variance=None, mask=None, g_loss=None, g_depth=None,
                         pow=2.0):
    """-> g_logp [B,D,H,W] (pdepth_dpv_soft_ce_backward_f32); count [B] is the forward's."""
    who = "dpv_soft_ce_backward"
    if g_loss is None and g_depth is None:
        raise RuntimeError(f"{who}: no incoming gradient")
    (B, D, H, W), logp, d_candi, label, depth_gt, mask, var, pw = _soft_ce_args(who, logp, d_candi, label, depth_gt, variance, mask, pow)
    _shape(count, (B,), "count", who)
    if g_loss is not None:
        _shape(g_loss, (B,), "g_loss", who)
        g_loss = _grad(g_loss, "g_loss")
    if g_depth is not None:
        _shape(g_depth, (B, H, W), "g_depth", who)
        g_depth = _grad(g_depth, "g_depth")
    count = count.contiguous()
    out = torch.empty_like(logp)
    _call("pdepth_dpv_soft_ce_backward_f32", logp.device, logp.data_ptr(), d_candi.data_ptr(), _ptr(label), _ptr(depth_gt), var, pw,
          _ptr(mask), _dev(count, "count"), B, D, H, W, _ptr(g_loss), _ptr(g_depth), out.data_ptr())
    return out


# ---- consistency and smoothness terms of the training loss (ops.depth_stereo_consistency ...) ----------------------------------
def _count_and_gradient(who, B, count, g_value):
    """(count, g_value) of a loss term's backward, each [B]: the forward's count and the gradient of its value."""
    _shape(count, (B,), "count", who)
    _shape(g_value, (B,), "g_value", who)
    return _tensors(who, count=count, g_value=g_value)


def _map_dims(who, t, name, least=2):
    if t.dim() != 3:
        raise RuntimeError(f"{who}: {name} must be [B,H,W], got {list(t.shape)}")
    B, H, W = t.shape
    if B < 1 or H < least or W < least:
        raise RuntimeError(f"{who}: {name} must be [B,H,W] with B >= 1 and H, W >= {least}, got {list(t.shape)}")
    return B, H, W


def _terms_out(B, H, W, dev, rows=2):
    """(out [rows,B], workspace | None, its bytes) of a loss-term forward."""
    return (torch.empty((rows, B), dtype=torch.float32, device=dev), *_workspace(_ask("pdepth_loss_terms_workspace_bytes", B, H, W), dev))


def _dsc_args(who, src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr):
    B, H, W = _map_dims(who, tgt_depth, "tgt_depth")
    _shape(src_depth, (B, H, W), "src_depth", who)
    _shape(src_mask, (B, H, W), "src_mask", who)
    _shape(Kinv, (B, 3, 3), "Kinv", who)
    _shape(proj, (B, 3, 4), "proj", who)
    _shape(intr, (B, 3, 3), "intr", who)
    if tuple(pose_row.shape) not in ((B, 4), (1, 4)):
        raise RuntimeError(f"{who}: pose_row must be [{B}, 4] or [1, 4], got {list(pose_row.shape)}")
    batched = 1 if (pose_row.shape[0] == B and B > 1) else 0
    return (B, H, W), batched, _tensors(who, src_depth=src_depth, tgt_depth=tgt_depth, src_mask=src_mask, Kinv=Kinv, proj=proj,
                                     pose_row=pose_row, intr=intr)


def loss_dsc(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr):
    """-> (value [B], count [B]): pdepth_loss_dsc_f32 on the current stream, no host synchronisation."""
    who = "loss_dsc"
    _no_autograd(who, src_depth, tgt_depth)
    (B, H, W), batched, t = _dsc_args(who, src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr)
    dev = t[0].device
    out, ws, ws_bytes = _terms_out(B, H, W, dev)
    _call("pdepth_loss_dsc_f32", dev, *(x.data_ptr() for x in t[:6]), batched, t[6].data_ptr(), B, H, W, out[0].data_ptr(),
          out[1].data_ptr(), _ptr(ws), ws_bytes)
    return out[0], out[1]


def loss_dsc_backward(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, count, g_value, want_src=True, want_tgt=True,
                      deterministic=False):
    """-> (g_src_depth | None, g_tgt_depth | None), each [B,H,W]: pdepth_loss_dsc_backward_f32; deterministic:
    pdepth_loss_dsc_backward_det_f32 (g_src_depth as an order-independent sum; g_tgt_depth has the same bits either way)."""
    who = "loss_dsc_backward"
    (B, H, W), batched, t = _dsc_args(who, src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr)
    count, g_value = _count_and_gradient(who, B, count, g_value)
    dev = t[0].device
    g_src = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_src else None
    g_tgt = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_tgt else None
    args = (*(x.data_ptr() for x in t[:6]), batched, t[6].data_ptr(), count.data_ptr(), g_value.data_ptr(), B, H, W, _ptr(g_src), _ptr(g_tgt))
    if deterministic:
        ws, ws_bytes = _workspace(_ask("pdepth_loss_dsc_backward_det_workspace_bytes", B, H, W) if want_src else 0, dev)
        _call("pdepth_loss_dsc_backward_det_f32", dev, *args, _ptr(ws), ws_bytes)
    else:
        _call("pdepth_loss_dsc_backward_f32", dev, *args)
    return g_src, g_tgt


def _rsc_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
    B, H, W = _map_dims(who, tgt_depth, "tgt_depth")
    _shape(src_rgb, (B, 3, H, W), "src_rgb", who)
    _shape(tgt_rgb, (B, 3, H, W), "tgt_rgb", who)
    _shape(Kinv, (B, 3, 3), "Kinv", who)
    _shape(proj, (B, 3, 4), "proj", who)
    return (B, H, W), _tensors(who, src_rgb=src_rgb, tgt_rgb=tgt_rgb, tgt_depth=tgt_depth, Kinv=Kinv, proj=proj)


def loss_rsc(src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
    """-> (value [B], count [B]): pdepth_loss_rsc_f32 (count = pixels of the mask; the value divides by 3 count)."""
    who = "loss_rsc"
    _no_autograd(who, tgt_depth)
    (B, H, W), t = _rsc_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj)
    dev = t[0].device
    out, ws, ws_bytes = _terms_out(B, H, W, dev)
    _call("pdepth_loss_rsc_f32", dev, *(x.data_ptr() for x in t), B, H, W, out[0].data_ptr(), out[1].data_ptr(), _ptr(ws), ws_bytes)
    return out[0], out[1]


def loss_rsc_backward(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, count, g_value):
    """-> g_tgt_depth [B,H,W]: pdepth_loss_rsc_backward_f32."""
    who = "loss_rsc_backward"
    (B, H, W), t = _rsc_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj)
    count, g_value = _count_and_gradient(who, B, count, g_value)
    dev = t[0].device
    g = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _call("pdepth_loss_rsc_backward_f32", dev, *(x.data_ptr() for x in t), count.data_ptr(), g_value.data_ptr(), B, H, W, g.data_ptr())
    return g


def _check_md(who, md, noun=None, H=None, W=None):
    """The refusals a half-width shares among the SSIM, the census and the photometric term: md is one the kernels are built for,
    and, given H and W, they hold one `noun` ("window", "patch") of (2 md + 1)^2.  Two calls where the shapes are judged between."""
    if md not in SSIM_MD:
        raise NotImplementedError(f"{who}: md={md}: the HIP kernels are built for md = 1, 2 and 3")
    if noun is not None and (H < 2 * md + 1 or W < 2 * md + 1):
        raise RuntimeError(f"{who}: H={H}, W={W}: a {noun} of md={md} needs H and W of at least {2 * md + 1}")


def _photo_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj, md):
    """_rsc_args, and the window of the SSIM: md one of SSIM_MD, H and W of at least 2 md + 1."""
    _check_md(who, md)
    _, H, W = _map_dims(who, tgt_depth, "tgt_depth")
    _check_md(who, md, "window", H, W)
    return _rsc_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj)


def loss_photo(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, ssim_weight, md=1):
    """-> (value [B], count [B]): pdepth_loss_photo_f32, the warp, the masked L1 and the SSIM distance in one pass (count = pixels
    of the mask)."""
    who = "loss_photo"
    _no_autograd(who, tgt_depth)
    (B, H, W), t = _photo_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj, md)
    dev = t[0].device
    ws, ws_bytes = _workspace(_ask("pdepth_loss_photo_workspace_bytes", B, H, W), dev)
    out = torch.empty((2, B), dtype=torch.float32, device=dev)
    _call("pdepth_loss_photo_f32", dev, *(x.data_ptr() for x in t), B, H, W, float(ssim_weight), md, out[0].data_ptr(), out[1].data_ptr(),
          _ptr(ws), ws_bytes)
    return out[0], out[1]


def loss_photo_backward(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, count, g_value, ssim_weight, md=1):
    """-> g_tgt_depth [B,H,W]: pdepth_loss_photo_backward_f32."""
    who = "loss_photo_backward"
    (B, H, W), t = _photo_args(who, src_rgb, tgt_rgb, tgt_depth, Kinv, proj, md)
    count, g_value = _count_and_gradient(who, B, count, g_value)
    dev = t[0].device
    g = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _call("pdepth_loss_photo_backward_f32", dev, *(x.data_ptr() for x in t), count.data_ptr(), g_value.data_ptr(), B, H, W,
          float(ssim_weight), md, g.data_ptr())
    return g


def _dc_args(who, large, small):
    B, H, W = _map_dims(who, large, "large", least=4)
    _shape(small, (B, H // 4, W // 4), "small", who)
    return (B, H, W), _tensors(who, large=large, small=small)


def loss_dc(large, small):
    """-> (value [B], count [B]): pdepth_loss_dc_f32."""
    who = "loss_dc"
    _no_autograd(who, large, small)
    (B, H, W), (large, small) = _dc_args(who, large, small)
    dev = large.device
    out, ws, ws_bytes = _terms_out(B, H // 4, W // 4, dev)
    _call("pdepth_loss_dc_f32", dev, large.data_ptr(), small.data_ptr(), B, H, W, out[0].data_ptr(), out[1].data_ptr(), _ptr(ws), ws_bytes)
    return out[0], out[1]


def loss_dc_backward(large, small, count, g_value, want_large=True, want_small=True):
    """-> (g_large [B,H,W] | None, g_small [B,H/4,W/4] | None): pdepth_loss_dc_backward_f32."""
    who = "loss_dc_backward"
    (B, H, W), (large, small) = _dc_args(who, large, small)
    count, g_value = _count_and_gradient(who, B, count, g_value)
    g_large = torch.empty_like(large) if want_large else None
    g_small = torch.empty_like(small) if want_small else None
    _call("pdepth_loss_dc_backward_f32", large.device, large.data_ptr(), small.data_ptr(), count.data_ptr(), g_value.data_ptr(), B, H, W,
          _ptr(g_large), _ptr(g_small))
    return g_large, g_small


def _smooth_args(who, depth, rgb):
    B, H, W = _map_dims(who, depth, "depth")
    if tuple(rgb.shape) != (B, 3, H, W):
        raise RuntimeError(f"{who}: rgb must be {[B, 3, H, W]}, the size of the depth map, got {list(rgb.shape)}; the multi-scale form "
                           "is loss_blocks.edge_aware_smoothness_loss")
    return (B, H, W), _tensors(who, depth=depth, rgb=rgb)


def loss_smooth(depth, rgb):
    """-> value [B]: pdepth_loss_smooth_f32."""
    who = "loss_smooth"
    _no_autograd(who, depth)
    (B, H, W), (depth, rgb) = _smooth_args(who, depth, rgb)
    dev = depth.device
    out, ws, ws_bytes = _terms_out(B, H, W, dev, rows=1)
    _call("pdepth_loss_smooth_f32", dev, depth.data_ptr(), rgb.data_ptr(), B, H, W, out.data_ptr(), _ptr(ws), ws_bytes)
    return out[0]


def loss_smooth_backward(depth, rgb, g_value):
    """-> g_depth [B,H,W]: pdepth_loss_smooth_backward_f32."""
    who = "loss_smooth_backward"
    (B, H, W), (depth, rgb) = _smooth_args(who, depth, rgb)
    _shape(g_value, (B,), "g_value", who)
    (g_value,) = _tensors(who, g_value=g_value)
    g = torch.empty_like(depth)
    _call("pdepth_loss_smooth_backward_f32", depth.device, depth.data_ptr(), rgb.data_ptr(), g_value.data_ptr(), B, H, W, g.data_ptr())
    return g


# ---- SSIM (ops.ssim) ---------------------------------------------------------------------------------------------------------------
SSIM_MD = (1, 2, 3)   # the window half-widths the kernels are built for


def _ssim_args(who, x, y, md):
    """((B, C, H, W), x, y) of an SSIM call: two [B,C,H,W] device tensors of one shape, as contiguous fp32."""
    _check_md(who, md)
    x, y = _tensors(who, x=x, y=y)
    if x.dim() != 4 or x.shape != y.shape:
        raise RuntimeError(f"{who}: x and y must be two [B,C,H,W] tensors of one shape, got {list(x.shape)} and {list(y.shape)}")
    B, C, H, W = x.shape
    if B < 1 or C < 1:
        raise RuntimeError(f"{who}: x and y must be [B,C,H,W] with B, C >= 1, got {list(x.shape)}")
    _check_md(who, md, "window", H, W)
    return (B, C, H, W), x, y


def ssim(x, y, md=1):
    """x, y [B,C,H,W] -> dist [B,C,H-2md,W-2md]: pdepth_ssim_f32 on the current stream."""
    who = "ssim"
    _no_autograd(who, x, y)
    (B, C, H, W), x, y = _ssim_args(who, x, y, md)
    out = torch.empty((B, C, H - 2 * md, W - 2 * md), dtype=torch.float32, device=x.device)
    _call("pdepth_ssim_f32", x.device, x.data_ptr(), y.data_ptr(), B, C, H, W, md, out.data_ptr())
    return out


def ssim_backward(x, y, g_out, md=1, want_x=True, want_y=True):
    """g_out [B,C,H-2md,W-2md] -> (g_x [B,C,H,W] | None, g_y [B,C,H,W] | None): pdepth_ssim_backward_f32."""
    who = "ssim_backward"
    (B, C, H, W), x, y = _ssim_args(who, x, y, md)
    _shape(g_out, (B, C, H - 2 * md, W - 2 * md), "g_out", who)
    (g_out,) = _tensors(who, g_out=g_out)
    if not (want_x or want_y):
        raise RuntimeError(f"{who}: no gradient requested")
    g_x = torch.empty_like(x) if want_x else None
    g_y = torch.empty_like(y) if want_y else None
    _call("pdepth_ssim_backward_f32", x.device, x.data_ptr(), y.data_ptr(), g_out.data_ptr(), B, C, H, W, md, _ptr(g_x), _ptr(g_y))
    return g_x, g_y


# ---- ternary census distance (ops.ternary) ------------------------------------------------------------------------------------------
TERNARY_MD = (1, 2, 3)   # the patch half-widths the kernels are built for


def _ternary_args(who, x, y, md):
    """((B, H, W), x, y) of a census call: two [B,3,H,W] device tensors of one shape, as contiguous fp32.  The shapes are judged
    first, where the tensors live; the device last."""
    _check_md(who, md)
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            _refuse(t, f"{who}: {name}")
    if x.dim() != 4 or x.shape != y.shape:
        raise RuntimeError(f"{who}: x and y must be two [B,3,H,W] tensors of one shape, got {list(x.shape)} and {list(y.shape)}")
    B, C, H, W = x.shape
    if B < 1 or C != 3:
        raise RuntimeError(f"{who}: x and y must be [B,3,H,W] RGB images with B >= 1, got {list(x.shape)} and {list(y.shape)}")
    _check_md(who, md, "patch", H, W)
    x, y = _tensors(who, x=x, y=y)
    return (B, H, W), x, y


def ternary(x, y, md=1):
    """x, y [B,3,H,W] -> dist [B,1,H,W]: pdepth_ternary_f32 on the current stream."""
    who = "ternary"
    _no_autograd(who, x, y)
    (B, H, W), x, y = _ternary_args(who, x, y, md)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    _call("pdepth_ternary_f32", x.device, x.data_ptr(), y.data_ptr(), B, H, W, md, out.data_ptr())
    return out


def ternary_backward(x, y, g_out, md=1, want_x=True, want_y=True):
    """g_out [B,1,H,W] -> (g_x [B,3,H,W] | None, g_y [B,3,H,W] | None): pdepth_ternary_backward_f32."""
    who = "ternary_backward"
    (B, H, W), x, y = _ternary_args(who, x, y, md)
    _shape(g_out, (B, 1, H, W), "g_out", who)
    (g_out,) = _tensors(who, g_out=g_out)
    if not (want_x or want_y):
        raise RuntimeError(f"{who}: no gradient requested")
    g_x = torch.empty_like(x) if want_x else None
    g_y = torch.empty_like(y) if want_y else None
    _call("pdepth_ternary_backward_f32", x.device, x.data_ptr(), y.data_ptr(), g_out.data_ptr(), B, H, W, md, _ptr(g_x), _ptr(g_y))
    return g_x, g_y


# ---- range map and occlusion mask (ops.range_map, ops.occlusion_mask, ops.depth_occlusion) -----------------------------------------
def _range_call(who, entry, head, B, H, W, th, want_range, want_visible, dev):
    """Outputs and workspace of a range-map entry, the call on the current stream: (range | None, visible | None), each [B,1,H,W]."""
    th = float(th)
    if th != th:
        raise RuntimeError(f"{who}: th is NaN")
    if not (want_range or want_visible):
        raise RuntimeError(f"{who}: no output requested")
    rng = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_range else None
    vis = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_visible else None
    ws, ws_bytes = _workspace(_ask("pdepth_range_map_workspace_bytes", B, H, W), dev)
    if ws is None:
        raise RuntimeError(f"{who}: B={B}, H={H}, W={W}: H*W must be at most 2^24 and B at most 65535")
    _call(entry, dev, *head, B, H, W, th, _ptr(rng), _ptr(vis), _ptr(ws), ws_bytes)
    return rng, vis


def range_map(coords, th=0.2, want_range=True, want_visible=False):
    """coords [B,2,H,W] un-normalised (x, y) -> (range [B,1,H,W] | None, visible [B,1,H,W] | None): pdepth_range_map_f32 on the
    current stream, no host synchronisation."""
    who = "range_map"
    _no_autograd(who, coords)
    if not isinstance(coords, torch.Tensor):
        _refuse(coords, f"{who}: coords")
    if coords.dim() != 4 or coords.shape[1] != 2 or min(coords.shape) < 1:
        raise RuntimeError(f"{who}: coords must be [B,2,H,W] with B, H, W >= 1, got {list(coords.shape)}")
    B, _, H, W = coords.shape
    (coords,) = _tensors(who, "insist", coords=coords)
    return _range_call(who, "pdepth_range_map_f32", (coords.data_ptr(),), B, H, W, th, want_range, want_visible, coords.device)


def depth_range_map(depth, Kinv, proj, src_mask=None, th=0.2, want_range=True, want_visible=False):
    """depth [B,H,W] of the source view (+ src_mask [B,H,W]), Kinv [B,3,3], proj [B,3,4] -> (range | None, visible | None), each
    [B,1,H,W]: pdepth_depth_range_map_f32 on the current stream, no host synchronisation."""
    who = "depth_range_map"
    _no_autograd(who, depth, src_mask, Kinv, proj)
    if not isinstance(depth, torch.Tensor):
        _refuse(depth, f"{who}: depth")
    B, H, W = _map_dims(who, depth, "depth")
    _shape(Kinv, (B, 3, 3), "Kinv", who)
    _shape(proj, (B, 3, 4), "proj", who)
    named = {"depth": depth, "Kinv": Kinv, "proj": proj}
    if src_mask is not None:
        _shape(src_mask, (B, H, W), "src_mask", who)
        named["src_mask"] = src_mask
    t = _tensors(who, "insist", **named)
    head = (t[0].data_ptr(), _ptr(t[3] if src_mask is not None else None), t[1].data_ptr(), t[2].data_ptr())
    return _range_call(who, "pdepth_depth_range_map_f32", head, B, H, W, th, want_range, want_visible, t[0].device)


# ---- flow_warp, the forward-backward check and the flow's smoothness (ops.flow_warp, ops.flow_fb_check, ops.smooth_grad_1st) -----
FLOW_PADS = {"border": 0, "zeros": 1}


def _flow_args(who, x, flow, pad, xname="x", fname="flow"):
    """((B, C, H, W), x, flow, pad code) of a flow_warp call: x [B,C,H,W] and flow [B,2,H,W], contiguous fp32 device tensors.  The
    shapes are judged first, where the tensors live; the device last."""
    if pad not in FLOW_PADS:
        raise RuntimeError(f"{who}: pad must be 'border' or 'zeros', got {pad!r}")
    for name, t in ((xname, x), (fname, flow)):
        if not isinstance(t, torch.Tensor):
            _refuse(t, f"{who}: {name}")
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{who}: {xname} must be [B,C,H,W] with B, C >= 1, got {list(x.shape)}")
    B, C, H, W = x.shape
    if H < 2 or W < 2:
        raise RuntimeError(f"{who}: H={H}, W={W}: the grid is normalised by H - 1 and W - 1, both must be at least 2")
    _shape(flow, (B, 2, H, W), fname, who)
    x, flow = _tensors(who, "insist", **{xname: x, fname: flow})
    return (B, C, H, W), x, flow, FLOW_PADS[pad]


def flow_warp(x, flow, pad="border"):
    """x [B,C,H,W] sampled at base grid + flow [B,2,H,W] -> [B,C,H,W]: pdepth_flow_warp_f32 on the current stream."""
    who = "flow_warp"
    _no_autograd(who, x, flow)
    (B, C, H, W), x, flow, code = _flow_args(who, x, flow, pad)
    out = torch.empty_like(x)
    _call("pdepth_flow_warp_f32", x.device, x.data_ptr(), flow.data_ptr(), B, C, H, W, code, out.data_ptr())
    return out


def flow_warp_backward(x, flow, grad_out, pad="border", want_x=True, want_flow=True, deterministic=False):
    """-> (grad_x [B,C,H,W] | None, grad_flow [B,2,H,W] | None): pdepth_flow_warp_backward_f32; deterministic:
    pdepth_flow_warp_backward_det_f32 (grad_x as an order-independent sum; grad_flow has the same bits either way)."""
    who = "flow_warp_backward"
    (B, C, H, W), x, flow, code = _flow_args(who, x, flow, pad)
    _shape(grad_out, (B, C, H, W), "grad_out", who)
    (grad_out,) = _tensors(who, "insist", grad_out=grad_out)
    if not (want_x or want_flow):
        raise RuntimeError(f"{who}: no gradient requested")
    dev = x.device
    g_x = torch.empty_like(x) if want_x else None
    g_f = torch.empty_like(flow) if want_flow else None
    args = (x.data_ptr(), flow.data_ptr(), grad_out.data_ptr(), B, C, H, W, code, _ptr(g_x), _ptr(g_f))
    if deterministic:
        ws, ws_bytes = _workspace(_ask("pdepth_flow_warp_backward_det_workspace_bytes", B, C, H, W) if want_x else 0, dev)
        _call("pdepth_flow_warp_backward_det_f32", dev, *args, _ptr(ws), ws_bytes)
    else:
        _call("pdepth_flow_warp_backward_f32", dev, *args)
    return g_x, g_f


def flow_fb_check(flow12, flow21, scale=0.01, bias=0.5):
    """flow12, flow21 [B,2,H,W] -> occ [B,1,H,W] (1 = the forward-backward check fails): pdepth_flow_fb_check_f32."""
    who = "flow_fb_check"
    _no_autograd(who, flow12, flow21)
    if isinstance(flow12, torch.Tensor) and (flow12.dim() != 4 or flow12.shape[1] != 2):
        raise RuntimeError(f"{who}: flow12 must be [B,2,H,W], got {list(flow12.shape)}")
    (B, _, H, W), flow12, flow21, _ = _flow_args(who, flow12, flow21, "zeros", xname="flow12", fname="flow21")
    occ = torch.empty((B, 1, H, W), dtype=torch.float32, device=flow12.device)
    _call("pdepth_flow_fb_check_f32", flow12.device, flow12.data_ptr(), flow21.data_ptr(), B, H, W, float(scale), float(bias),
          occ.data_ptr())
    return occ


def _cost_volume_args(who, x1, x2, flow, max_displacement, negative_slope, pad):
    """((B, C, H, W), x1, x2, flow | None, md, slope, pad code) of a cost-volume call: x1, x2 [B,C,H,W] and flow [B,2,H,W] or None,
    contiguous fp32 device tensors.  Shapes and scalars are judged first, where the tensors live; the device last."""
    if pad not in FLOW_PADS:
        raise RuntimeError(f"{who}: pad must be 'border' or 'zeros', got {pad!r}")
    md, slope = int(max_displacement), float(negative_slope)
    if md != max_displacement or not 1 <= md <= 4:
        raise RuntimeError(f"{who}: max_displacement must be 1..4, got {max_displacement!r}")
    if not slope >= 0.0:
        raise RuntimeError(f"{who}: negative_slope is NaN or negative ({negative_slope!r})")
    named = {"x1": x1, "x2": x2} if flow is None else {"x1": x1, "x2": x2, "flow": flow}
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            _refuse(t, f"{who}: {name}")
    if x1.dim() != 4 or min(x1.shape) < 1:
        raise RuntimeError(f"{who}: x1 must be [B,C,H,W] with every size >= 1, got {list(x1.shape)}")
    B, C, H, W = x1.shape
    _shape(x2, (B, C, H, W), "x2", who)
    if flow is not None:
        if H < 2 or W < 2:
            raise RuntimeError(f"{who}: H={H}, W={W}: the grid is normalised by H - 1 and W - 1, both must be at least 2 with a flow")
        _shape(flow, (B, 2, H, W), "flow", who)
    t = _tensors(who, "insist", **named)
    return (B, C, H, W), t[0], t[1], (t[2] if flow is not None else None), md, slope, FLOW_PADS[pad]


def flow_cost_volume(x1, x2, flow=None, max_displacement=4, negative_slope=0.1, pad="border"):
    """leaky_relu(correlation(x1, flow_warp(x2, flow, pad))) -> [B, (2 md + 1)^2, H, W]: pdepth_flow_cost_volume_f32 on the current
    stream, one launch; flow None: no warp."""
    who = "flow_cost_volume"
    _no_autograd(who, x1, x2, flow)
    (B, C, H, W), x1, x2, flow, md, slope, code = _cost_volume_args(who, x1, x2, flow, max_displacement, negative_slope, pad)
    out = torch.empty((B, (2 * md + 1) ** 2, H, W), dtype=torch.float32, device=x1.device)
    _call("pdepth_flow_cost_volume_f32", x1.device, x1.data_ptr(), x2.data_ptr(), _ptr(flow), B, C, H, W, md, slope, code, out.data_ptr())
    return out


def flow_cost_volume_backward(x1, x2, flow, out, grad_out, max_displacement=4, negative_slope=0.1, pad="border", want_x1=True,
                              want_x2=True, want_flow=True, deterministic=False):
    """-> (grad_x1 | None, grad_x2 | None, grad_flow | None): pdepth_flow_cost_volume_backward_f32; deterministic:
    pdepth_flow_cost_volume_backward_det_f32 (grad_x2 as an order-independent sum; the others have the same bits either way).
    `out` is the forward's result.  The workspace (the gradient of the warped image, and the integer accumulator) is allocated here."""
    who = "flow_cost_volume_backward"
    (B, C, H, W), x1, x2, flow, md, slope, code = _cost_volume_args(who, x1, x2, flow, max_displacement, negative_slope, pad)
    nd2 = (2 * md + 1) ** 2
    _shape(out, (B, nd2, H, W), "out", who)
    _shape(grad_out, (B, nd2, H, W), "grad_out", who)
    out, grad_out = _tensors(who, "insist", out=out, grad_out=grad_out)
    want_flow = bool(want_flow) and flow is not None
    if not (want_x1 or want_x2 or want_flow):
        raise RuntimeError(f"{who}: no gradient requested")
    dev = x1.device
    g1 = torch.empty_like(x1) if want_x1 else None
    g2 = torch.empty_like(x2) if want_x2 else None
    gf = torch.empty_like(flow) if want_flow else None
    name = "pdepth_flow_cost_volume_backward_det" if deterministic else "pdepth_flow_cost_volume_backward"
    need = flow is not None and (want_x2 or want_flow)
    ws, ws_bytes = _workspace(_ask(name + "_workspace_bytes", B, C, H, W, 1) if need else 0, dev)
    _call(name + "_f32", dev, x1.data_ptr(), x2.data_ptr(), _ptr(flow), out.data_ptr(), grad_out.data_ptr(), B, C, H, W, md, slope, code,
          _ptr(g1), _ptr(g2), _ptr(gf), _ptr(ws), ws_bytes)
    return g1, g2, gf


def _flow_photo_args(who, im, other, flow, mask, w_l1, w_ssim, w_ternary, pad):
    """((B, H, W), (im, other, flow, mask), weights, pad code) of a flow_photo call: im, other [B,3,H,W], flow [B,2,H,W], mask
    [B,1,H,W], contiguous fp32 device tensors.  Shapes and scalars are judged first, where the tensors live; the device last."""
    if pad not in FLOW_PADS:
        raise RuntimeError(f"{who}: pad must be 'border' or 'zeros', got {pad!r}")
    named = {"im": im, "other": other, "flow": flow, "mask": mask}
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            _refuse(t, f"{who}: {name}")
    if im.dim() != 4 or im.shape[0] < 1 or im.shape[1] != 3:
        raise RuntimeError(f"{who}: im must be [B,3,H,W] with B >= 1, got {list(im.shape)}")
    B, _, H, W = im.shape
    weights = (float(w_l1), float(w_ssim), float(w_ternary))
    if H < 2 or W < 2:
        raise RuntimeError(f"{who}: H={H}, W={W}: the grid is normalised by H - 1 and W - 1, both must be at least 2")
    if (weights[1] > 0 or weights[2] > 0) and (H < 3 or W < 3):
        raise RuntimeError(f"{who}: H={H}, W={W}: the SSIM and census terms need H and W of at least 3")
    _shape(other, (B, 3, H, W), "other", who)
    _shape(flow, (B, 2, H, W), "flow", who)
    _shape(mask, (B, 1, H, W), "mask", who)
    return (B, H, W), tuple(_tensors(who, "insist", **named)), weights, FLOW_PADS[pad]


def flow_photo(im, other, flow, mask, w_l1, w_ssim, w_ternary, pad="border"):
    """-> (value, count), 0-dim tensors: pdepth_flow_photo_f32, the warp of `other` along the flow, the masked L1, the SSIM and the
    census distance against `im` in one pass, over the mean of the mask (count = its sum)."""
    who = "flow_photo"
    _no_autograd(who, im, other, flow, mask)
    (B, H, W), t, weights, code = _flow_photo_args(who, im, other, flow, mask, w_l1, w_ssim, w_ternary, pad)
    dev = t[0].device
    ws, ws_bytes = _workspace(_ask("pdepth_flow_photo_workspace_bytes", B, H, W), dev)
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    _call("pdepth_flow_photo_f32", dev, *(x.data_ptr() for x in t), B, H, W, code, *weights, out[0].data_ptr(), out[1].data_ptr(),
          _ptr(ws), ws_bytes)
    return out[0], out[1]


def flow_photo_backward(im, other, flow, mask, count, g_value, w_l1, w_ssim, w_ternary, pad="border"):
    """count, g_value (one element each) -> g_flow [B,2,H,W]: pdepth_flow_photo_backward_f32."""
    who = "flow_photo_backward"
    (B, H, W), t, weights, code = _flow_photo_args(who, im, other, flow, mask, w_l1, w_ssim, w_ternary, pad)
    for name, v in (("count", count), ("g_value", g_value)):
        if v.numel() != 1:
            raise RuntimeError(f"{who}: {name} must have one element, got {list(v.shape)}")
    count, g_value = _tensors(who, count=count.reshape(1), g_value=g_value.reshape(1))
    dev = t[0].device
    g = torch.empty_like(t[2])
    _call("pdepth_flow_photo_backward_f32", dev, *(x.data_ptr() for x in t), count.data_ptr(), g_value.data_ptr(), B, H, W, code, *weights,
          g.data_ptr())
    return g


def _smooth1_args(who, flo, image):
    for name, t in (("flo", flo), ("image", image)):
        if not isinstance(t, torch.Tensor):
            _refuse(t, f"{who}: {name}")
    if flo.dim() != 4 or image.dim() != 4 or min(flo.shape) < 1 or min(image.shape) < 1 or \
            (flo.shape[0],) + tuple(flo.shape[2:]) != (image.shape[0],) + tuple(image.shape[2:]):
        raise RuntimeError(f"{who}: flo [B,Cf,H,W] and image [B,Ci,H,W] must share B, H and W, got {list(flo.shape)} and {list(image.shape)}")
    B, Cf, H, W = flo.shape
    if H < 2 or W < 2:
        raise RuntimeError(f"{who}: H={H}, W={W}: both must be at least 2")
    flo, image = _tensors(who, "insist", flo=flo, image=image)
    return (B, Cf, image.shape[1], H, W), flo, image


def loss_smooth1(flo, image, alpha):
    """-> value (a 0-dim tensor): pdepth_loss_smooth1_f32."""
    who = "loss_smooth1"
    _no_autograd(who, flo)
    (B, Cf, Ci, H, W), flo, image = _smooth1_args(who, flo, image)
    dev = flo.device
    ws, ws_bytes = _workspace(_ask("pdepth_loss_terms_workspace_bytes", B, H, W), dev)
    out = torch.empty((1,), dtype=torch.float32, device=dev)
    _call("pdepth_loss_smooth1_f32", dev, flo.data_ptr(), image.data_ptr(), B, Cf, Ci, H, W, float(alpha), out.data_ptr(), _ptr(ws), ws_bytes)
    return out[0]


def loss_smooth1_backward(flo, image, alpha, g_value):
    """g_value (one element) -> g_flo [B,Cf,H,W]: pdepth_loss_smooth1_backward_f32."""
    who = "loss_smooth1_backward"
    (B, Cf, Ci, H, W), flo, image = _smooth1_args(who, flo, image)
    if g_value.numel() != 1:
        raise RuntimeError(f"{who}: g_value must have one element, got {list(g_value.shape)}")
    (g_value,) = _tensors(who, g_value=g_value.reshape(1))
    g = torch.empty_like(flo)
    _call("pdepth_loss_smooth1_backward_f32", flo.device, flo.data_ptr(), image.data_ptr(), g_value.data_ptr(), B, Cf, Ci, H, W,
          float(alpha), g.data_ptr())
    return g


# ---- evaluation metrics (ops.depth_metrics) -----------------------------------------------------------------------------------
def depth_metrics(truth, pred=None, logp=None, d_candi=None, mask=None, clamp_max=None, want_depth=False):
    """truth [B,H,W] + (pred [B,H,W] | logp [B,D,H,W], d_candi [D]) [+ mask [B,H,W]] -> (metrics [B,9], count [B], depth [B,H,W] |
    None): pdepth_depth_metrics_f32 on the current stream, no host synchronisation.  clamp_max None or <= 0: no clamp."""
    who = "depth_metrics"
    _no_autograd(who, truth, pred, logp, mask)
    if (pred is None) == (logp is None):
        raise RuntimeError(f"{who}: give exactly one prediction, pred [B,H,W] or logp [B,D,H,W]")
    if truth.dim() != 3:
        raise RuntimeError(f"{who}: truth must be [B,H,W]")
    B, H, W = truth.shape
    D = 0
    if logp is not None:
        if logp.dim() != 4:
            raise RuntimeError(f"{who}: logp must be [B,D,H,W]")
        D = logp.shape[1]
        _shape(logp, (B, D, H, W), "logp", who)
        if d_candi is None or d_candi.numel() != D:
            raise RuntimeError(f"{who}: d_candi has {0 if d_candi is None else d_candi.numel()} entries, volume has D={D}")
    else:
        _shape(pred, (B, H, W), "pred", who)
        if want_depth:
            raise RuntimeError(f"{who}: want_depth belongs to the volume form (the depth map form is given its map)")
    if mask is not None:
        _shape(mask, (B, H, W), "mask", who)
    truth, pred, logp, d_candi, mask = _optional(truth=truth, pred=pred, logp=logp, d_candi=d_candi if logp is not None else None, mask=mask)
    dev = truth.device
    out = torch.empty(B * 10, dtype=torch.float32, device=dev)
    metrics, count = out[:B * 9].view(B, 9), out[B * 9:]
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth else None
    ws, ws_bytes = _workspace(_ask("pdepth_depth_metrics_workspace_bytes", B, H, W), dev)
    _call("pdepth_depth_metrics_f32", dev, _ptr(logp), _ptr(pred), _ptr(d_candi), truth.data_ptr(), _ptr(mask),
          float(clamp_max) if clamp_max is not None else 0.0, B, D, H, W, metrics.data_ptr(), count.data_ptr(), _ptr(depth), _ptr(ws), ws_bytes)
    return metrics, count, depth


# ---- flow evaluation (ops.flow_metrics, ops.flow_resize) ------------------------------------------------------------------------
def flow_metrics(gt, pred, move_mask=None, want_flow=False):
    """gt [B,2|4,H,W], pred [B,2,h,w] [, move_mask [B,H,W]] -> (errors [B,8], counts [B,5], flow_up [B,2,H,W] | None):
    pdepth_flow_metrics_f32 on the current stream, no host synchronisation."""
    who = "flow_metrics"
    _no_autograd(who, gt, pred, move_mask)
    if gt.dim() != 4 or gt.shape[1] not in (2, 4):
        raise RuntimeError(f"{who}: gt must be [B,2,H,W] or [B,4,H,W], got {list(gt.shape)}")
    B, C, H, W = gt.shape
    if pred.dim() != 4 or pred.shape[0] != B or pred.shape[1] != 2:
        raise RuntimeError(f"{who}: pred must be [{B}, 2, h, w], got {list(pred.shape)}")
    h, w = pred.shape[2:]
    if move_mask is not None:
        if C != 4:
            raise RuntimeError(f"{who}: a move mask needs a truth of 4 channels (it multiplies valid)")
        _shape(move_mask, (B, H, W), "move_mask", who)
    gt, pred, move_mask = _optional(gt=gt, pred=pred, move_mask=move_mask)
    dev = gt.device
    if pred.device != dev or (move_mask is not None and move_mask.device != dev):
        raise RuntimeError(f"{who}: gt, pred and move_mask must be on one device")
    out = torch.empty(B * 13, dtype=torch.float32, device=dev)
    errors, counts = out[:B * 8].view(B, 8), out[B * 8:].view(B, 5)
    flow_up = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if want_flow else None
    ws, ws_bytes = _workspace(_ask("pdepth_flow_metrics_workspace_bytes", B, H, W), dev)
    _call("pdepth_flow_metrics_f32", dev, gt.data_ptr(), C, pred.data_ptr(), h, w, _ptr(move_mask), B, H, W, errors.data_ptr(),
          counts.data_ptr(), _ptr(flow_up), _ptr(ws), ws_bytes)
    return errors, counts, flow_up


def flow_resize(flow, size, align_corners=False):
    """flow [B,2,h,w] -> [B,2,H,W], rescaled by W / w and H / h and resized: pdepth_flow_resize_f32 on the current stream."""
    who = "flow_resize"
    _no_autograd(who, flow)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise RuntimeError(f"{who}: flow must be [B,2,h,w], got {list(flow.shape)}")
    B, _, h, w = flow.shape
    H, W = (int(s) for s in size)
    (flow,) = _tensors(None, flow=flow)
    out = torch.empty((B, 2, H, W), dtype=torch.float32, device=flow.device)
    _call("pdepth_flow_resize_f32", flow.device, flow.data_ptr(), B, h, w, H, W, 1 if align_corners else 0, out.data_ptr())
    return out


# ---- ground truth from LiDAR (ops.lidar_depth) ----------------------------------------------------------------------------------
def lidar_depth(points, counts, M_velo2cam, intr, height, width, filtering=2, filterdiff=1.0, pool_default=1000.0):
    """points [B,Nmax,4|3], counts [B] int32, M_velo2cam [4,4] | [B,4,4], intr [3,4] | [B,3,4] -> (dmap [B,H,W], mask [B,H,W],
    dmap_quarter [B,H//4,W//4], mask_quarter [B,H//4,W//4]): pdepth_lidar_depth_f32 on the current stream, no host
    synchronisation."""
    who = "lidar_depth"
    _no_autograd(who, points, M_velo2cam, intr)
    if points.dim() != 3 or points.shape[2] not in (3, 4):
        raise RuntimeError(f"{who}: points must be [B,Nmax,4] or [B,Nmax,3], got {tuple(points.shape)}")
    B, Nmax, dim = points.shape
    _shape(counts, (B,), "counts", who)
    if M_velo2cam.dim() not in (2, 3) or intr.dim() not in (2, 3):
        raise RuntimeError(f"{who}: M_velo2cam must be [4,4] or [B,4,4] and intr [3,4] or [B,3,4]")
    _shape(M_velo2cam, (4, 4) if M_velo2cam.dim() == 2 else (B, 4, 4), "M_velo2cam", who)
    _shape(intr, (3, 4) if intr.dim() == 2 else (B, 3, 4), "intr", who)
    H, W = int(height), int(width)
    points, counts, M_velo2cam, intr = _tensors(None, None, points=points, counts=counts, M_velo2cam=M_velo2cam, intr=intr)
    for nm, t, dtype in (("counts", counts, torch.int32), ("points", points, torch.float32), ("M_velo2cam", M_velo2cam, torch.float32),
                         ("intr", intr, torch.float32)):   # (every device before any dtype, the counts' before the floats')
        if t.dtype != dtype:
            _refuse(t, nm, dtype)
    dev = points.device
    ws, ws_bytes = _workspace(_ask("pdepth_lidar_depth_workspace_bytes", B, H, W), dev)
    large = torch.empty((2, B, max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
    small = torch.empty((2, B, max(H, 0) // 4, max(W, 0) // 4), dtype=torch.float32, device=dev)
    _call("pdepth_lidar_depth_f32", dev, _ptr(points) or None, counts.data_ptr(), M_velo2cam.data_ptr(), intr.data_ptr(), B, Nmax, dim,
          int(M_velo2cam.dim() == 3), int(intr.dim() == 3), H, W, int(filtering), float(filterdiff), float(pool_default),
          large[0].data_ptr() or None, large[1].data_ptr() or None, small[0].data_ptr() or None, small[1].data_ptr() or None,
          _ptr(ws), ws_bytes)
    return large[0], large[1], small[0], small[1]
