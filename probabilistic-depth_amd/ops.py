"""Batched entry points of the hot path (thin, typed wrappers over ``_native``).

These are what the host model and the harness call; the reference-compatible per-item
functions in ``warping.homography`` / ``utils.img_utils`` are wrappers around them.
All tensors are fp32 device tensors; nothing here runs on the CPU.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native

METRICS = {"L2": _native.METRIC_L2, "L1": _native.METRIC_L1}
# "tiled1" / "tiled2" / "dist" / "direct" force one of the implementations behind "auto" (parity tests, A/B timing);
# "cells" / "mfma" / "corr" name retired kernels: the keys stay so that such a call fails with the library's message
ALGOS = {"auto": _native.ALGO_AUTO, "direct": _native.ALGO_DIRECT, "tiled1": _native.ALGO_TILED_1,
         "tiled2": _native.ALGO_TILED_2, "cells": _native.ALGO_CELLS, "mfma": _native.ALGO_MFMA, "corr": _native.ALGO_CORR, "dist": _native.ALGO_DIST}
BLAS_MODES = {"fma": _native.BLAS_FMA, "separate": _native.BLAS_SEPARATE, None: None}


def _metric(feat_dist):
    if feat_dist not in METRICS:
        # same error as warping/homography.py:133
        raise Exception("undefined metric for feature distance ...")
    return METRICS[feat_dist]


_D_CANDI_CACHE = {}


def d_candi_tensor(d_candi, device):
    """float64 numpy / list / tensor -> fp32 device tensor (homography.py:115 cast).

    Host arrays are uploaded once per (values, device) and cached: the candidates are a constant of a run, and a
    pageable host-to-device copy per op would synchronise the stream (and cannot be captured in a HIP graph)."""
    if isinstance(d_candi, torch.Tensor):
        return d_candi.to(device=device, dtype=torch.float32)
    import numpy as np
    arr = np.ascontiguousarray(np.asarray(d_candi), dtype=np.float32)
    dev = torch.device(device)
    key = (arr.tobytes(), dev.type, dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else -1))
    t = _D_CANDI_CACHE.get(key)
    if t is None:
        if len(_D_CANDI_CACHE) > 64:
            _D_CANDI_CACHE.clear()
        t = torch.from_numpy(arr.copy()).to(dev)
        _D_CANDI_CACHE[key] = t
    return t


def _deterministic(flag):
    """The `deterministic` keyword of the ops with a scattered gradient: None follows torch.use_deterministic_algorithms()."""
    return torch.are_deterministic_algorithms_enabled() if flag is None else bool(flag)


def sweep_cost(ref, src, K, R, t, rays, cxcy, d_candi, sigma, feat_dist="L2", algo="auto", blas=None, deterministic=None):
    """cost [B,D,H,W].  Batched est_swp_volume_v4 (warping/homography.py:98-135).

    blas: None = reproduce the rounding of THIS host's CPU BLAS (see _native.host_blas_mode),
    "fma" / "separate" to force one (golden fixtures record the mode of the host that made them).
    deterministic (backward only; the forward and its values are the same either way): True sums the gradient of src as
    64-bit integers (csrc/sweep_bwd_det.hip: the same bits from run to run, 8 bytes of workspace per element of src), False
    with float atomics, None = torch.are_deterministic_algorithms_enabled() when the op is called.
    """
    if _sweep_wants_grad("sweep_cost", ref, src, K, R, t, rays, cxcy, d_candi):
        dc = d_candi_tensor(d_candi, ref.device)
        cost, _, _ = _SweepFn.apply(ref, src, K, R, t, rays, cxcy, dc, sigma, _metric(feat_dist), ALGOS[algo], BLAS_MODES[blas],
                                    True, False, False, _deterministic(deterministic))
        return cost
    cost, _, _ = _native.sweep(ref, src, K, R, t, rays, cxcy, d_candi_tensor(d_candi, ref.device), sigma,
                               _metric(feat_dist), ALGOS[algo], want_cost=True, blas_mode=BLAS_MODES[blas])
    return cost


def sweep_dpv(ref, src, K, R, t, rays, cxcy, d_candi, sigma, feat_dist="L2", algo="auto",
              want_cost=False, want_logp=True, want_depth=True, blas=None, deterministic=None):
    """Fused sweep -> log_softmax(dim=1) -> E[d].  Returns (cost|None, logp|None, depth|None).

    models/packnet.py:380-394 + utils/img_utils.py:52-61 in one kernel.  deterministic: as sweep_cost.
    """
    if _sweep_wants_grad("sweep_dpv", ref, src, K, R, t, rays, cxcy, d_candi):
        dc = d_candi_tensor(d_candi, ref.device)
        return _SweepFn.apply(ref, src, K, R, t, rays, cxcy, dc, sigma, _metric(feat_dist), ALGOS[algo], BLAS_MODES[blas],
                              want_cost, want_logp, want_depth, _deterministic(deterministic))
    return _native.sweep(ref, src, K, R, t, rays, cxcy, d_candi_tensor(d_candi, ref.device), sigma,
                         _metric(feat_dist), ALGOS[algo], want_cost=want_cost, want_logp=want_logp,
                         want_depth=want_depth, blas_mode=BLAS_MODES[blas])


UnsupportedShape = _native.UnsupportedShape


def pack_source(src, n_planes=64, algo="auto", feat_dist="L2"):
    """Source views [B,V,C,H,W] -> the sweep kernels' staging layout, once (pdepth_pack_source_f32); pass the result as
    `src` to sweep_cost / sweep_dpv with the same algo and feat_dist (the kernel they select decides whether the layout is
    mean-centred).  The re-layout is 10 % of a fused sweep call.  Raises UnsupportedShape for shapes the packed sweep does
    not take."""
    return _native.pack_source(src, n_planes, ALGOS[algo], _metric(feat_dist))


def pack_views(feat, rgb, n_views, n_planes=64):
    """Encoder epilogue: cat(feat, avg_pool2d(rgb)) -> (packed source views, NCHW reference view) in one pass
    (pdepth_pack_views_f32; models/models.py:518-534).  Pass the PackedSource as `src` and the tensor as `ref` to
    sweep_cost / sweep_dpv.  Raises UnsupportedShape for shapes the packed sweep does not take (callers use cat + avg_pool2d)."""
    return _native.pack_views(feat, rgb, n_views, n_planes)


def dpv_reduce(logits, d_candi, want_logp=True, want_depth=True, inplace=False):
    """(logp, depth) from logits [B,D,H,W]: log_softmax(dim=1) + dpv_to_depthmap(BV_log=True).

    d_candi may be None when only the log-softmax is wanted (want_depth=False).
    fp16 / bf16 logits (torch.autocast) are widened in the kernel's load: logp and depth are fp32, the gradient comes back in the
    logits' dtype, and inplace is ignored, the output being another type.
    """
    if d_candi is None:
        if want_depth:
            raise RuntimeError("dpv_reduce: d_candi is required for the depth output")
        dc = torch.zeros(logits.shape[1], dtype=torch.float32, device=logits.device)
    else:
        dc = d_candi_tensor(d_candi, logits.device)
    if _wants_grad(logits):
        _refuse_grad("dpv_reduce", d_candi=d_candi)
        out = _DpvReduceFn.apply(logits, None, dc, want_logp, False, want_depth, False, False, False, None)
        return out[0], out[2]
    return _native.dpv_reduce(logits, dc, want_logp, want_depth, inplace)


def dpv_reduce_ex(logits, d_candi=None, addend=None, want_logp=True, want_prob=False, want_depth=False, want_var=False,
                  want_quarter=False, inplace=False, prob_dtype=None):
    """One pass over (logits [+ addend]): log_softmax over D and any of exp(logp), E[d], Var[d], the nearest
    quarter-resolution log-DPV (the next frame's prev_output).  Returns a dict with the requested outputs.

    Mixed precision: fp16 / bf16 logits (and an addend of the same dtype; another dtype raises) are widened to fp32 in the
    kernel's load and every sum is the fp32 one.  The outputs are fp32; prob is fp32 (prob_dtype=None) or, with
    prob_dtype=logits.dtype, the fp32 value rounded once to that dtype (what a conv under autocast would make of it).  inplace
    is ignored for half logits: the output is another type.  Gradients come back in the dtype of logits and addend.

    models/models.py:694 + :697 (feedback update and decoder input), trainer/default_trainer.py:333-336 (variance),
    :221 (prev_output)."""
    if d_candi is None:
        if want_depth or want_var:
            raise RuntimeError("dpv_reduce_ex: d_candi is required for the depth / variance outputs")
        dc = torch.zeros(logits.shape[1], dtype=torch.float32, device=logits.device)
    else:
        dc = d_candi_tensor(d_candi, logits.device)
    if _wants_grad(logits, addend):
        _refuse_grad("dpv_reduce_ex", d_candi=d_candi)
        out = _DpvReduceFn.apply(logits, addend, dc, want_logp, want_prob, want_depth, want_var, want_quarter, True, prob_dtype)
        return {k: v for k, v in zip(("logp", "prob", "depth", "var", "quarter"), out) if v is not None}
    return _native.dpv_reduce_ex(logits, dc, addend, want_logp, want_prob, want_depth, want_var, want_quarter, inplace, prob_dtype)


def ufield(dpv, d_candi, intr, mask=None, BV_log=True, unc_ang=5, z_start=0.6, z_end=0.9, min_depth=0.0, quash=False):
    """Uncertainty-field collapse, batched: (plane [B,D,W], masked depth [B,H,W]) of a (log-)DPV [B,D,H,W]
    (utils/img_utils.py:268-358).  mask [B,H,W] | [B,1,H,W] | None."""
    if mask is not None and mask.dim() == 4:
        mask = mask[:, 0]
    if unc_ang != 0 and dpv.dim() == 4 and (dpv.shape[2] == 1 or dpv.shape[3] == 1):
        # the reference's convert_flowfield divides by size - 1 (utils/img_utils.py:170-176) and fails the same way
        raise ZeroDivisionError("ufield: a shift (unc_ang != 0) needs H, W >= 2: the sampling grid divides by size - 1")
    # depth of rows shifted in from outside the image = dpv_to_depthmap of the zero padding = the fp32 sum of the candidates:
    # formed on the host when the candidates come from the host (no device synchronisation inside the call)
    d_sum = None
    if not isinstance(d_candi, torch.Tensor):
        import numpy as np
        d_sum = float(torch.from_numpy(np.ascontiguousarray(np.asarray(d_candi), dtype=np.float32)).sum())
    return _native.ufield(dpv, d_candi_tensor(d_candi, dpv.device), intr, mask, BV_log, unc_ang, z_start, z_end, min_depth, quash,
                          d_sum=d_sum)


def dpv_expect(dpv, d_candi, BV_log=False):
    """depth [B,H,W] from a (log-)DPV [B,D,H,W] (utils/img_utils.py:52-61, batched)."""
    if _wants_grad(dpv):
        _refuse_grad("dpv_expect", d_candi=d_candi)
        return _DpvExpectFn.apply(dpv, d_candi_tensor(d_candi, dpv.device), bool(BV_log))
    return _native.dpv_expect(dpv, d_candi_tensor(d_candi, dpv.device), BV_log)


def dpv_soft_ce(logp, d_candi, label=None, depth_gt=None, variance=None, mask=None, want_depth=False, pow=2.0):
    """Soft-label cross-entropy of a log-DPV [B,D,H,W] over the depth axis, per item, fused with the expectation:
    (loss [B], depth [B,H,W] | None).  soft_cross_entropy_loss(BV_log=True) for the whole batch (losses/loss_blocks.py:186-202)
    + dpv_to_depthmap (utils/img_utils.py:52-61) in one pass over the volume.

    The label is `label` [B,D,H,W] or, given `depth_gt` [B,H,W] and `variance`, what gen_soft_label_torch(d_candi, depth_gt,
    variance, zero_invalid=True, pow) would build (utils/img_utils.py:24-47) -- formed in the kernel, never stored.
    mask [B,H,W] | [B,1,H,W] | None: loss[b] = sum(ce * mask) / #(mask == 1), 0 for an item without a valid pixel (decided on
    the device).  Differentiable with respect to logp only; depth equals dpv_expect(logp, d_candi, BV_log=True) bit for bit."""
    if mask is not None and mask.dim() == 4:
        mask = mask[:, 0]
    dc = d_candi_tensor(d_candi, logp.device)
    if _wants_grad(logp):
        _refuse_grad("dpv_soft_ce", label=label, depth_gt=depth_gt, mask=mask, d_candi=d_candi)
        return _DpvSoftCeFn.apply(logp, dc, label, depth_gt, variance, mask, bool(want_depth), float(pow))
    loss, _, depth = _native.dpv_soft_ce(logp, dc, label, depth_gt, variance, mask, want_depth, pow)
    return loss, depth


# the devkit's names in its order (external/deval_lib/src/evaluate_depth.h:125-133): the columns of depth_metrics
DEPTH_METRIC_NAMES = ("mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log", "abs relative",
                      "squared relative")


def depth_metrics(truth, pred=None, logp=None, d_candi=None, mask=None, clamp_max=None, want_depth=False):
    """The KITTI devkit's nine depth errors per item, on the device: (metrics [B,9] in the order of DEPTH_METRIC_NAMES, count [B]
    = the number of valid pixels, depth [B,H,W] | None).  The tail of the evaluation loop (trainer/default_trainer.py:247-256)
    composed with img_utils.depth_error (utils/img_utils.py:17-22) and depthError (external/deval_lib/src/evaluate_depth.h:20-121)
    for the whole batch, without copying a depth map to the host.

    The prediction is `pred` [B,H,W] or, given `logp` [B,D,H,W] and `d_candi`, the expectation of the log-DPV, formed from one
    read of the volume (the bits of dpv_expect(logp, d_candi, BV_log=True); want_depth returns that map from the same pass).
    truth [B,H,W]; mask [B,H,W] | [B,1,H,W] | None multiplies the prediction; clamp_max (the trainer: d_candi[-1]) replaces every
    truth >= clamp_max, None = no clamp; a truth of 0 becomes -1.

    The reference's argument order is kept: depth_error(predicted, truth) hands its arguments to depthError(D_gt, D_ipol) in
    that order, so a pixel is valid where the masked PREDICTION is > 0 (0 and NaN are not) and the two relative errors divide by
    the PREDICTION, not by the ground truth.  A valid pixel whose truth is 0 or negative makes the log and inverse metrics of its
    item NaN; an item without a valid pixel (the reference throws) has nine NaNs and count 0.  Not differentiable."""
    if mask is not None and mask.dim() == 4:
        mask = mask[:, 0]
    dc = d_candi_tensor(d_candi, logp.device) if (logp is not None and d_candi is not None) else None
    return _native.depth_metrics(truth, pred=pred, logp=logp, d_candi=dc, mask=mask, clamp_max=clamp_max, want_depth=want_depth)


# the columns of flow_metrics' errors: evaluate_flow's values in its order (utils/flow_utils.py:117-121), then the two rates it
# accumulates for the move mask and does not return
FLOW_METRIC_NAMES = ("epe", "epe_noc", "epe_occ", "fl", "epe_move", "epe_static", "fl_move", "fl_static")


def flow_metrics(gt, pred, move_mask=None, want_flow=False):
    """The flow evaluation per item, on the device: (errors [B,8] in the order of FLOW_METRIC_NAMES, counts [B,5] = the sums of
    valid, noc, valid - noc, valid * move, valid * (1 - move), flow_up [B,2,H,W] | None).  utils/flow_utils.evaluate_flow
    (utils/flow_utils.py:61-123) for the whole batch, without copying the prediction to the host.

    gt [B,2,H,W] = (u, v) or [B,4,H,W] = (u, v, valid, noc); pred [B,2,h,w] of any size; move_mask [B,H,W] | [B,1,H,W] | None
    (4-channel truth only).  The prediction is rescaled (u / w * W, v / h * H in float, in that order) and resized to H x W with
    cv2.resize's INTER_LINEAR rule (half-pixel centres, no antialiasing); want_flow returns that map from the same pass and
    changes no bit of the rest.  epe = |flow_up - gt_uv|; a 2-channel truth gives its plain mean in column 0; a 4-channel truth
    the means over valid, noc and valid - noc (the last divided by max(sum, 1)) and fl = 100 * #(epe * valid > 3 and
    epe * valid / max(|gt_uv|, 1e-10) > 0.05) / sum(valid); the move mask adds columns 4 to 7.  A column the inputs do not
    define is NaN, and so is a mean over no pixel.  Sums are float64 in a fixed order: the same bits from call to call.  Not
    differentiable."""
    if isinstance(move_mask, torch.Tensor) and move_mask.dim() == 4:
        move_mask = move_mask[:, 0]
    _refuse_grad("flow_metrics", gt=gt, pred=pred, move_mask=move_mask)
    return _native.flow_metrics(gt, pred, move_mask=move_mask, want_flow=want_flow)


def flow_resize(flow, size, align_corners=False):
    """flow [B,2,h,w] -> [B,2,H,W] for size = (H, W): every tap rescaled (u / w * W, v / h * H), then the bilinear sample.
    align_corners=False: cv2.resize's INTER_LINEAR rule, the bits of flow_metrics' flow_up; True: the coordinates of
    F.interpolate(align_corners=True), what utils/flow_utils.resize_flow computes (utils/flow_utils.py:50-58).  Not differentiable."""
    _refuse_grad("flow_resize", flow=flow)
    return _native.flow_resize(flow, size, align_corners=align_corners)


def lidar_depth(points, counts, M_velo2cam, intr, width, height, filtering=2, filterdiff=1.0, pool=4, pool_default=1000.0):
    """The ground truth of a batch from its LiDAR scans, on the device: generate_depth (external/utils_lib/python/utils_lib.cpp:
    86-160, upsample = 0) for every item, then the loader's quarter-resolution map and masks (kittiloader/kitti.py:683-729), in
    one call on the current stream without a host synchronisation.

    points [B,Nmax,4] = (x, y, z, w) or [B,Nmax,3] (w = 1); counts [B] int32: rows at or beyond counts[b] are ignored, 0 gives
    all-zero maps; M_velo2cam [4,4] | [B,4,4]; intr [3,4] | [3,3] | [B,3,4] | [B,3,3] (a 3x3 gets the zero column the loader
    appends), all fp32 -- cast float64 calibration with .float(), as the reference's binding does.  A point is transformed and
    projected in fp32, kept iff cam.z >= 0.1, lands in pixel ((int)(u_f - 0.5), (int)(v_f - 0.5)) (truncation toward zero), and
    the pixel takes the minimum cam.z; the filter clears a pixel when another pixel of its (2 filtering + 1)^2 window is nearer by
    more than filterdiff, and the last filtering + 1 rows and columns (include/pdepth.h has every detail).
    Returns {"dmap_imgsizes" [B,H,W], "masks_imgsizes" [B,1,H,W], "dmaps" [B,H//4,W//4], "masks" [B,1,H//4,W//4]}: the keys
    BaseLoss(labels_from_depth=True), harness.validate_step and nmode default_upsample read.  Not differentiable."""
    if pool != 4:
        raise NotImplementedError(f"lidar_depth: pool = {pool}: the kernel pools 4x4 blocks (the loader's resize_dmap = 0.25)")
    _refuse_grad("lidar_depth", points=points, M_velo2cam=M_velo2cam, intr=intr)
    if intr.shape[-1] == 3:
        intr = torch.cat([intr, intr.new_zeros(intr.shape[:-1] + (1,))], dim=-1)
    dmap, mask, dmap_q, mask_q = _native.lidar_depth(points, counts, M_velo2cam, intr, height, width, filtering, filterdiff,
                                                     pool_default)
    return {"dmap_imgsizes": dmap, "masks_imgsizes": mask.unsqueeze(1), "dmaps": dmap_q, "masks": mask_q.unsqueeze(1)}


def depth_stereo_consistency(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, deterministic=None):
    """depth_stereo_consistency_loss per item (losses/loss_blocks.py:147-171), one HIP pass: (value [B], count [B]).

    src_depth, tgt_depth [B,H,W] | [B,1,H,W]; src_mask likewise; Kinv [B,3,3] = intr^-1 and proj [B,3,4] = intr @ pose_target2src[:3]
    as utils.inverse_warp.warp_with_matrices takes them; pose_row [B,4] | [1,4] = the third row of the source-to-target pose; intr
    [B,3,3].  The mask (valid & lower two thirds & warped > 0) is formed from the sample positions of the HIP inverse_warp, bit for
    bit; count is its size per item, not differentiable; an item with an empty mask is NaN.  Differentiable with respect to both
    depth maps (the source through an atomic scatter; deterministic, as sweep_cost's: an order-independent integer sum instead,
    csrc/scatter_det.hip); everything else is data."""
    who = "depth_stereo_consistency"
    src_depth, tgt_depth, src_mask = (_squeeze_map(t) for t in (src_depth, tgt_depth, src_mask))
    if _wants_grad(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr):
        _refuse_data_grad(who, src_mask=src_mask, Kinv=Kinv, proj=proj, pose_row=pose_row, intr=intr)
        return _DscFn.apply(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, _deterministic(deterministic))
    return _native.loss_dsc(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr)


def rgb_stereo_consistency(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, ssim_weight=0.0, ssim_md=1):
    """rgb_stereo_consistency_loss per item (losses/loss_blocks.py:114-145), one HIP pass: (value [B], count [B]).

    src_rgb, tgt_rgb [B,3,H,W]; tgt_depth [B,H,W] | [B,1,H,W]; Kinv, proj as above.  count = the pixels of the mask (valid & lower
    two thirds); the value divides by 3 count.  Differentiable with respect to tgt_depth only, through the sample position.

    ssim_weight = w != 0: the photometric term, warp, L1 and SSIM in one pass each way (csrc/photo.hip), with m the mask
        (1 - w) sum_c sum(|tgt_c m - warped_c m| m) / (3 count) + w mean(SSIM(warped m, tgt m, ssim_md)) / mean(m),
    what loss_blocks.rgb_stereo_consistency_loss(..., ssim_weight=w, ssim_md=ssim_md, per_item=True) composes; ssim_md = 1, 2 or 3
    (another: NotImplementedError; H or W below 2 ssim_md + 1: a RuntimeError that names the sizes).  The backward is a gather in a
    fixed order: the same bits from call to call.  With w == 0 the call is the L1 pass it has always been, and ssim_md is ignored."""
    who = "rgb_stereo_consistency"
    tgt_depth = _squeeze_map(tgt_depth)
    if ssim_weight == 0:
        if _wants_grad(src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
            _refuse_data_grad(who, src_rgb=src_rgb, tgt_rgb=tgt_rgb, Kinv=Kinv, proj=proj)
            return _RscFn.apply(src_rgb, tgt_rgb, tgt_depth, Kinv, proj)
        return _native.loss_rsc(src_rgb, tgt_rgb, tgt_depth, Kinv, proj)
    w, md = float(ssim_weight), int(ssim_md)
    if _wants_grad(src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
        _refuse_data_grad(who, src_rgb=src_rgb, tgt_rgb=tgt_rgb, Kinv=Kinv, proj=proj)
        return _PhotoFn.apply(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, w, md)
    return _native.loss_photo(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, w, md)


def depth_consistency(large, small):
    """depth_consistency_loss per item (losses/loss_blocks.py:173-184), one HIP pass: (value [B], count [B]).  large [B,H,W], small
    [B,H//4,W//4]; differentiable with respect to both."""
    if _wants_grad(large, small):
        return _DcFn.apply(large, small)
    return _native.loss_dc(large, small)


def edge_aware_smoothness(depth, rgb):
    """edge_aware_smoothness_loss at one scale, per item (losses/loss_blocks.py:73-112), one HIP pass: value [B].  depth [B,H,W] |
    [B,1,H,W], rgb [B,3,H,W] of the same size (another size -- the multi-scale form -- is
    loss_blocks.edge_aware_smoothness_loss); differentiable with respect to depth only."""
    who = "edge_aware_smoothness"
    depth = _squeeze_map(depth)
    if depth.dim() != 3 or rgb.dim() != 4 or tuple(rgb.shape) != (depth.shape[0], 3) + tuple(depth.shape[1:]):
        raise RuntimeError(f"{who}: depth {list(depth.shape)} and rgb {list(rgb.shape)} must be [B,H,W] and [B,3,H,W] of one size; "
                           "for an image of another size use loss_blocks.edge_aware_smoothness_loss")
    if _wants_grad(depth, rgb):
        _refuse_data_grad(who, rgb=rgb)
        return _SmoothFn.apply(depth, rgb)
    return _native.loss_smooth(depth, rgb)


def ssim(x, y, md=1):
    """SSIM distance of two images (losses/loss_blocks.py:47-66), one HIP pass: x, y [B,C,H,W] -> clamp((1 - SSIM) / 2, 0, 1)
    [B,C,H-2md,W-2md], one value per (2 md + 1)^2 window, md = 1, 2 or 3 (another md: NotImplementedError; H or W below 2 md + 1: a
    RuntimeError that names the sizes).  The inputs go through .float().contiguous().  Where x and y are equal bit for bit the
    result is exactly 0.  Differentiable with respect to x and / or y (csrc/ssim.hip: a gather, the same bits from call to call);
    the kernel is asked only for the gradients that are needed, and the forward under autograd is the no-grad kernel call."""
    md = int(md)
    if _wants_grad(x, y):
        return _SsimFn.apply(x, y, md)
    return _native.ssim(x, y, md)


def ternary(x, y, md=1):
    """Ternary census distance of two RGB images (losses/loss_blocks.py:8-44), one HIP pass: x, y [B,3,H,W] -> [B,1,H,W], the mean
    over the (2 md + 1)^2 offsets o of d / (0.1 + d), d = (n_o - n'_o)^2, n_o = t_o / sqrt(0.81 + t_o^2), t_o = I(p+o) - I(p) on the
    grayscale times 255; 0 within md of a border.  md = 1, 2 or 3 (another md: NotImplementedError; C != 3, or H or W below
    2 md + 1: a RuntimeError that names the shapes).  The inputs go through .float().contiguous().  Where x and y are equal bit for
    bit the result and both gradients are exactly 0.  Differentiable with respect to x and / or y (csrc/ternary.hip: a gather, the
    same bits from call to call); the kernel is asked only for the gradients that are needed, and the forward under autograd is
    the no-grad kernel call."""
    md = int(md)
    if _wants_grad(x, y):
        return _TernaryFn.apply(x, y, md)
    return _native.ternary(x, y, md)


def range_map(coords):
    """Range map of a forward splat (utils/warp_utils.py:25-79, get_corresponding_map), three HIP launches (clear, splat, convert): coords
    [B,2,H,W], un-normalised (x, y) positions of the source pixels, fp32 -> [B,1,H,W], the bilinear mass every pixel receives.  Only
    in-bounds taps count; a NaN or infinite position adds nothing.  The sum is an order-independent integer sum (csrc/occlusion.hip):
    the same bits from call to call.  Not differentiable: coords that require grad are refused."""
    _refuse_grad("range_map", coords=coords)
    return _native.range_map(coords)[0]


def occlusion_mask(coords, th=0.2, want_range=False):
    """visible [B,1,H,W]: 0 where the range map of coords, clamped to [0, 1], is below th -- where no source pixel lands -- and 1
    elsewhere: 1 - get_occu_mask_backward's mask (utils/warp_utils.py:102-108) for coords = base grid + flow.  want_range: (visible,
    range), both from one convert pass.  coords as ops.range_map takes them; a constant, without a graph."""
    _refuse_grad("occlusion_mask", coords=coords)
    rng, vis = _native.range_map(coords, th=th, want_range=bool(want_range), want_visible=True)
    return (vis, rng) if want_range else vis


def depth_occlusion(src_depth, Kinv, proj, th=0.2, src_mask=None, want_range=False):
    """The visibility mask of the view a source depth map is splatted into: src_depth [B,H,W] | [B,1,H,W], src_mask likewise or
    None (a pixel whose mask is 0 adds nothing), Kinv [B,3,3] and proj [B,3,4] as utils.inverse_warp.warp_with_matrices takes them
    for the warp whose target is the source view.  A source pixel lands where that warp samples it -- the same chain, bit for bit --
    so the mask describes the warp the consistency term of the opposite direction performs.  -> visible [B,1,H,W] (1 = seen), or
    (visible, range) with want_range.  The mask is a constant: the inputs are detached (src_depth may require grad) and the result
    carries no graph."""
    who = "depth_occlusion"
    for name, t in (("src_depth", src_depth), ("Kinv", Kinv), ("proj", proj)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name}: expected a torch.Tensor")
    src_depth, src_mask = (_squeeze_map(t) for t in (src_depth, src_mask))
    detached = [t.detach() if isinstance(t, torch.Tensor) else t for t in (src_depth, Kinv, proj, src_mask)]
    rng, vis = _native.depth_range_map(detached[0], detached[1], detached[2], src_mask=detached[3], th=th, want_range=bool(want_range),
                                       want_visible=True)
    return (vis, rng) if want_range else vis


def flow_warp(x, flow, pad="border", deterministic=None):
    """flow_warp of the flow loss and the flow network (utils/warp_utils.py:82-89), one HIP pass: x [B,C,H,W] sampled bilinearly at
    base grid + flow [B,2,H,W] (channel 0 along x), pad 'border' or 'zeros', with the reference's normalisation (2 v / (W - 1) - 1
    into grid_sample's align_corners=False).  fp32 device tensors.  A non-finite position gives 0 in both paddings.  Differentiable
    with respect to x and / or flow (csrc/flow_warp.hip): grad_flow is a per-owner sum, the same bits from call to call; grad_x is a
    scatter -- float atomics, or with deterministic=True an order-independent integer sum (None follows
    torch.are_deterministic_algorithms_enabled() at the call)."""
    if _wants_grad(x, flow):
        return _FlowWarpFn.apply(x, flow, pad, _deterministic(deterministic))
    return _native.flow_warp(x, flow, pad)


def flow_cost_volume(x1, x2, flow=None, max_displacement=4, negative_slope=0.1, pad="border", deterministic=None):
    """The flow network's per-level cost volume (models/pwclite.py), one HIP pass: leaky_relu(correlation(x1, flow_warp(x2, flow,
    pad)), negative_slope) -> [B, (2 md + 1)^2, H, W], the correlation with kernel 1, strides 1 and pad_size = max_displacement
    (1..4); flow None: no warp (the coarsest level).  fp32 device tensors, the dtype policy of flow_warp.  Neither the warped image
    nor the pre-activation volume is written (csrc/cost_volume.hip).  Differentiable with respect to x1, x2 and the flow: a gather
    for grad_x1 and the gradient of the warped image, then flow_warp's own backward -- grad_x2 a scatter (float atomics, or with
    deterministic=True the order-independent integer sum; None follows torch.are_deterministic_algorithms_enabled() at the call),
    grad_flow a per-owner sum."""
    if _wants_grad(x1, x2, flow):
        return _FlowCostVolumeFn.apply(x1, x2, flow, max_displacement, negative_slope, pad, _deterministic(deterministic))
    return _native.flow_cost_volume(x1, x2, flow, max_displacement, negative_slope, pad)


def flow_photometric(im, other, flow, mask, w_l1, w_ssim, w_ternary, pad="border"):
    """One direction of the flow loss's photometric term (losses/flow_loss.py:13-27 with the warp of :66-78 inside), one HIP pass
    each way (csrc/flow_photo.hip): -> (value, count), 0-dim fp32 tensors.  im, other [B,3,H,W], flow [B,2,H,W], mask [B,1,H,W],
    fp32 device tensors.  With R = flow_warp(other, flow, pad), x = R mask, y = im mask:
        value = (w_l1 mean(|im - R| mask) + w_ssim mean(ssim(x, y)) + w_ternary mean(ternary(x, y))) / mean(mask),  count = sum(mask)
    what unFlowLoss.loss_photomatric composes from ops.flow_warp, ops.ssim and ops.ternary (md = 1).  A weight that is not > 0
    removes its term entirely; H or W below 3 with the SSIM or census term on: a RuntimeError that names the sizes.  A NaN behind
    a zero mask makes the value NaN, an empty mask gives 0 / 0 = NaN, a non-finite flow samples 0.  Differentiable with respect to
    the flow only (a gather in a fixed order: the same bits from call to call, no deterministic switch needed); im, other and mask
    are data and are refused when they require grad."""
    who = "flow_photometric"
    if _wants_grad(im, other, flow, mask):
        for name, x in (("im", im), ("other", other), ("mask", mask)):
            if isinstance(x, torch.Tensor) and x.requires_grad:
                raise RuntimeError(f"{who}: {name} requires grad, but the HIP backward differentiates the flow only (images and "
                                   f"masks are data); detach {name}")
        return _FlowPhotoFn.apply(im, other, flow, mask, float(w_l1), float(w_ssim), float(w_ternary), pad)
    return _native.flow_photo(im, other, flow, mask, w_l1, w_ssim, w_ternary, pad)


def flow_fb_check(flow12, flow21, scale=0.01, bias=0.5):
    """Forward-backward check (utils/warp_utils.py:92-99, get_occu_mask_bidirection), one HIP pass: occ [B,1,H,W], 1 where
    |flow12 + w|^2 > scale (|flow12|^2 + |w|^2) + bias with w = flow21 sampled at base + flow12 (zeros padding).  A mask has no
    gradient: the flows are detached and the result carries no graph, as the reference's .float() of a comparison."""
    detached = [t.detach() if isinstance(t, torch.Tensor) else t for t in (flow12, flow21)]
    return _native.flow_fb_check(detached[0], detached[1], scale, bias)


def smooth_grad_1st(flo, image, alpha):
    """smooth_grad_1st (losses/loss_blocks.py:210-220), one HIP pass and a fixed-order sum: flo [B,Cf,H,W], image [B,Ci,H,W] ->
    mean(wx |dx flo|) / 4 + mean(wy |dy flo|) / 4, wx = exp(-alpha mean_c |dx image|); a 0-dim tensor, the same bits from call to
    call.  Differentiable with respect to flo only (a per-owner gather); image is data."""
    if _wants_grad(flo, image):
        _refuse_data_grad("smooth_grad_1st", image=image)
        return _Smooth1Fn.apply(flo, image, float(alpha))
    return _native.loss_smooth1(flo, image, alpha)


def dpv_moments(dpv, d_candi, BV_log=True):
    """(mean, variance) [B,H,W] of the depth distribution of a (log-)DPV (trainer/default_trainer.py:333-336)."""
    return _native.dpv_moments(dpv, d_candi_tensor(d_candi, dpv.device), BV_log)


def warp_feature(src, K, R, t, rays, cxcy, d_candi, blas=None, differentiable=False, deterministic=None):
    """[B,V,D,H,W] diagonal warp (warping/homography.py:137-168, batched).

    differentiable=False (the default): the no-grad kernel call, which refuses a src that requires grad while grad mode is on.
    differentiable=True: when src requires grad the call runs under autograd -- the same forward kernel, bit for bit, and the
    backward of csrc/warp_bwd.hip with respect to src (the geometry and the candidates are data and are refused when they
    require grad); when nothing requires grad it is the no-grad call.
    deterministic: the gradient of src as an order-independent integer sum (bit-reproducible) instead of float atomics,
    None = torch.are_deterministic_algorithms_enabled() when the op is called."""
    dc = d_candi_tensor(d_candi, src.device)
    if differentiable:
        _refuse_grad("warp_feature", K=K, R=R, t=t, rays=rays, cxcy=cxcy, d_candi=d_candi)
        if _wants_grad(src):
            return _WarpFeatureFn.apply(src, K, R, t, rays, cxcy, dc, BLAS_MODES[blas], _deterministic(deterministic))
    return _native.warp_feature(src, K, R, t, rays, cxcy, dc, blas_mode=BLAS_MODES[blas])


def sample_coords(K, R, t, rays, cxcy, d_candi, H, W, blas=None, algo=_native.ALGO_AUTO):
    return _native.sample_coords(K, R, t, rays, cxcy, d_candi_tensor(d_candi, K.device), H, W, algo=algo,
                                 blas_mode=BLAS_MODES[blas])


def dpv_fuse(logp, dmaps, masks, d_candi, var=0.3, eps=None, want_fused=True, want_log=True):
    """Bayesian fusion of a log-DPV with the Gaussian soft label of a sparse depth map.

    utils/img_utils.py:360-375 (gen_dpv_withmask) + models/models.py:666-672 in one kernel.
    masks may be [B,1,H,W] (reference layout, channel 0 is used) or [B,H,W].
    Returns (fused probabilities | None, log fused | None).  Differentiable with respect to logp only (csrc/dpv_fuse_bwd.hip);
    the depth maps, the masks and the candidates are data.
    """
    if eps is None:
        eps = torch.finfo(float).eps  # reference: utils/img_utils.py:12
    if masks.dim() == 4:
        masks = masks[:, 0]
    if _wants_grad(logp):
        _refuse_grad("dpv_fuse", dmaps=dmaps, masks=masks, d_candi=d_candi)
        return _DpvFuseFn.apply(logp, dmaps.float(), masks.float(), d_candi_tensor(d_candi, logp.device), float(var), float(eps),
                                bool(want_fused), bool(want_log))
    return _native.dpv_fuse(logp, dmaps.float(), masks.float(), d_candi_tensor(d_candi, logp.device), var, eps,
                            want_fused, want_log)


# ---- autograd ---------------------------------------------------------------------------------------------------------------
# The public functions above take the autograd path only when grad mode is on and a feature / volume input requires grad;
# every other call runs the no-grad code unchanged.  The Functions' forwards call the same _native forwards (same algo), so
# values are bit-identical to the no-grad call; their backwards are the HIP kernels of csrc/sweep_bwd.hip, csrc/dpv_bwd.hip,
# csrc/dpv_fuse_bwd.hip and csrc/warp_bwd.hip.  warp_feature alone takes that path only on request (differentiable=True: the model
# and the reference-signature wrapper pass it); its plain call keeps refusing a src that requires grad.
# Differentiable: the feature maps (ref, NCHW src), logits, addend, the DPV of dpv_expect, the log-DPV of dpv_fuse, the src of
# warp_feature.  Not differentiable: the geometry
# (K, R, t, rays, cxcy, d_candi -- the reference's training takes them from the data loader), which is refused when it
# requires grad.  Every backward is once_differentiable: a second-order gradient through a HIP backward raises, it is not a constant.

def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in tensors)


def _refuse_grad(who, **named):
    for name, x in named.items():
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who}: {name} requires grad, but the HIP backward differentiates the feature maps / volumes only "
                               f"(geometry and depth candidates are data); detach {name}")


def _squeeze_map(t):
    """[B,1,H,W] -> [B,H,W] (the reference's layout of depth maps and masks)."""
    return t[:, 0] if isinstance(t, torch.Tensor) and t.dim() == 4 and t.shape[1] == 1 else t


def _refuse_data_grad(who, **named):
    for name, x in named.items():
        if isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{who}: {name} requires grad, but the HIP backward differentiates the depth maps only "
                               f"(images, masks, poses and intrinsics are data); detach {name}")


def _sweep_wants_grad(who, ref, src, K, R, t, rays, cxcy, d_candi):
    """True if this sweep call runs under autograd; raises for inputs the backward cannot differentiate."""
    if not torch.is_grad_enabled():
        return False
    _refuse_grad(who, K=K, R=R, t=t, rays=rays, cxcy=cxcy, d_candi=d_candi)
    if isinstance(src, _native.PackedSource):
        if isinstance(ref, torch.Tensor) and ref.requires_grad:
            raise RuntimeError(f"{who}: ref requires grad, but src is a PackedSource: the staging layout has no fp32 source to "
                               "differentiate; pass the NCHW features [B,V,C,H,W] as src")
        return False
    return _wants_grad(ref, src)


class _SweepFn(torch.autograd.Function):
    """sweep_cost / sweep_dpv under autograd: (cost | None, logp | None, depth | None) of the NCHW features.  logp is kept for
    the backward whenever logp or depth is returned (computed by the same fused call when the caller did not ask for it)."""

    @staticmethod
    def forward(ctx, ref, src, K, R, t, rays, cxcy, dc, sigma, metric, algo, blas_mode, want_cost, want_logp, want_depth, deterministic):
        ctx.set_materialize_grads(False)
        keep_logp = want_logp or want_depth
        cost, logp, depth = _native.sweep(ref, src, K, R, t, rays, cxcy, dc, sigma, metric, algo, want_cost=want_cost,
                                          want_logp=keep_logp, want_depth=want_depth, blas_mode=blas_mode)
        ctx.save_for_backward(ref, src, K, R, t, rays, cxcy, dc, logp if keep_logp else None)
        ctx.cfg = (sigma, metric, blas_mode, deterministic)
        return cost, (logp if want_logp else None), depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cost, g_logp, g_depth):
        ref, src, K, R, t, rays, cxcy, dc, logp = ctx.saved_tensors
        sigma, metric, blas_mode, deterministic = ctx.cfg
        g = None
        if g_logp is not None or g_depth is not None:
            g = _native.dpv_reduce_backward(logp, dc, g_logp=g_logp, g_depth=g_depth)
        if g_cost is not None:
            g = g_cost.float() if g is None else g + g_cost
        want_ref, want_src = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_ref = g_src = None
        if g is not None and (want_ref or want_src):
            g_ref, g_src = _native.sweep_backward(ref, src, K, R, t, rays, cxcy, dc, g, sigma, metric, want_ref=want_ref,
                                                  want_src=want_src, blas_mode=blas_mode, deterministic=deterministic)
        return (g_ref, g_src) + (None,) * 14


class _WarpFeatureFn(torch.autograd.Function):
    """warp_feature(differentiable=True) under autograd.  The warp is linear in src: the backward needs the geometry only, and
    returns a gradient in src's shape (an expanded view is summed over by autograd)."""

    @staticmethod
    def forward(ctx, src, K, R, t, rays, cxcy, dc, blas_mode, deterministic):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(K, R, t, rays, cxcy, dc)
        ctx.cfg = (blas_mode, deterministic)
        with torch.no_grad():   # (the kernel of the no-grad call: the same bits)
            return _native.warp_feature(src, K, R, t, rays, cxcy, dc, blas_mode=blas_mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        if g_out is None:
            return (None,) * 9
        K, R, t, rays, cxcy, dc = ctx.saved_tensors
        blas_mode, deterministic = ctx.cfg
        g = _native.warp_feature_backward(g_out.float().contiguous(), K, R, t, rays, cxcy, dc, blas_mode=blas_mode,
                                          deterministic=deterministic)
        return (g,) + (None,) * 8


class _DpvReduceFn(torch.autograd.Function):
    """dpv_reduce / dpv_reduce_ex under autograd: (logp, prob, depth, var, quarter), each None unless requested; var and
    quarter (the next frame's prev_output) are not differentiable.  inplace is not honoured: the outputs are new tensors.
    Half-precision logits: the saved logp is fp32, the gradient of logits and addend is stored in their dtype by the backward
    kernel, and a g_prob of prob's half dtype is read as it is."""

    @staticmethod
    def forward(ctx, logits, addend, dc, want_logp, want_prob, want_depth, want_var, want_quarter, ex, prob_dtype):
        ctx.set_materialize_grads(False)
        ctx.in_dtype = logits.dtype
        if ex:   # (the forward of the public function that was called: dpv_reduce_ex or dpv_reduce)
            out = _native.dpv_reduce_ex(logits, dc, addend, True, want_prob, want_depth, want_var, want_quarter, False, prob_dtype)
        else:
            lp, dep = _native.dpv_reduce(logits, dc, True, want_depth, False)
            out = {"logp": lp} if dep is None else {"logp": lp, "depth": dep}
        logp = out["logp"]
        ctx.save_for_backward(logp, dc)
        nd = [out[k] for k in ("var", "quarter") if k in out]
        if nd:
            ctx.mark_non_differentiable(*nd)
        return (logp if want_logp else None, out.get("prob"), out.get("depth"), out.get("var"), out.get("quarter"))

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logp, g_prob, g_depth, g_var, g_quarter):
        logp, dc = ctx.saved_tensors
        g = None
        if g_logp is not None or g_prob is not None or g_depth is not None:
            if ctx.in_dtype == torch.float32:
                g = _native.dpv_reduce_backward(logp, dc, g_logp=g_logp, g_prob=g_prob, g_depth=g_depth)
            else:
                g = _native.dpv_reduce_backward_lp(logp, dc, ctx.in_dtype, g_logp=g_logp, g_prob=g_prob, g_depth=g_depth)
        return (g if ctx.needs_input_grad[0] else None, g if ctx.needs_input_grad[1] else None) + (None,) * 8


class _DpvFuseFn(torch.autograd.Function):
    """dpv_fuse under autograd: (fused | None, log fused | None).  Nothing but the inputs is saved: the backward recomputes the
    prior and the unclamped posterior (a clamped plane's output no longer holds it)."""

    @staticmethod
    def forward(ctx, logp, dmaps, masks, dc, var, eps, want_fused, want_log):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(logp, dmaps, masks, dc)
        ctx.cfg = (var, eps)
        return _native.dpv_fuse(logp, dmaps, masks, dc, var, eps, want_fused, want_log)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_fused, g_logfused):
        if g_fused is None and g_logfused is None:
            return (None,) * 8
        logp, dmaps, masks, dc = ctx.saved_tensors
        g = _native.dpv_fuse_backward(logp, dmaps, masks, dc, ctx.cfg[0], ctx.cfg[1],
                                      None if g_fused is None else g_fused.contiguous(),
                                      None if g_logfused is None else g_logfused.contiguous())
        return (g,) + (None,) * 7


class _DpvExpectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dpv, dc, bv_log):
        ctx.save_for_backward(dpv, dc)
        ctx.bv_log = bv_log
        return _native.dpv_expect(dpv, dc, bv_log)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_depth):
        dpv, dc = ctx.saved_tensors
        return _native.dpv_expect_backward(dpv, dc, ctx.bv_log, g_depth), None, None


class _DpvSoftCeFn(torch.autograd.Function):
    """dpv_soft_ce under autograd: (loss, depth | None); the backward is one pass of csrc/loss.hip over the volume."""

    @staticmethod
    def forward(ctx, logp, dc, label, depth_gt, variance, mask, want_depth, pow):
        ctx.set_materialize_grads(False)
        loss, count, depth = _native.dpv_soft_ce(logp, dc, label, depth_gt, variance, mask, want_depth, pow)
        ctx.save_for_backward(logp, dc, count, label, depth_gt, mask)
        ctx.cfg = (variance, pow)
        return loss, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_depth):
        logp, dc, count, label, depth_gt, mask = ctx.saved_tensors
        g = None
        if g_loss is not None or g_depth is not None:
            g = _native.dpv_soft_ce_backward(logp, dc, count, label, depth_gt, ctx.cfg[0], mask, g_loss, g_depth, ctx.cfg[1])
        return (g,) + (None,) * 7


class _DscFn(torch.autograd.Function):
    """depth_stereo_consistency under autograd: (value, count); the backward recomputes every pixel from the inputs."""

    @staticmethod
    def forward(ctx, src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, deterministic):
        ctx.set_materialize_grads(False)
        ctx.deterministic = deterministic
        value, count = _native.loss_dsc(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr)
        ctx.save_for_backward(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr, count)
        ctx.mark_non_differentiable(count)
        return value, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_count):
        want_src, want_tgt = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_value is None or not (want_src or want_tgt):
            return (None,) * 8
        *inputs, count = ctx.saved_tensors
        g_src, g_tgt = _native.loss_dsc_backward(*inputs, count, g_value, want_src=want_src, want_tgt=want_tgt,
                                                 deterministic=ctx.deterministic)
        return (g_src, g_tgt) + (None,) * 6


class _RscFn(torch.autograd.Function):
    """rgb_stereo_consistency under autograd: (value, count)."""

    @staticmethod
    def forward(ctx, src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
        ctx.set_materialize_grads(False)
        value, count = _native.loss_rsc(src_rgb, tgt_rgb, tgt_depth, Kinv, proj)
        ctx.save_for_backward(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, count)
        ctx.mark_non_differentiable(count)
        return value, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_count):
        if g_value is None or not ctx.needs_input_grad[2]:
            return (None,) * 5
        return None, None, _native.loss_rsc_backward(*ctx.saved_tensors, g_value), None, None


class _PhotoFn(torch.autograd.Function):
    """rgb_stereo_consistency with the SSIM mixed in, under autograd: (value, count); the backward recomputes from the inputs."""

    @staticmethod
    def forward(ctx, src_rgb, tgt_rgb, tgt_depth, Kinv, proj, ssim_weight, md):
        ctx.set_materialize_grads(False)
        ctx.cfg = (ssim_weight, md)
        value, count = _native.loss_photo(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, ssim_weight, md)
        ctx.save_for_backward(src_rgb, tgt_rgb, tgt_depth, Kinv, proj, count)
        ctx.mark_non_differentiable(count)
        return value, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_count):
        if g_value is None or not ctx.needs_input_grad[2]:
            return (None,) * 7
        return None, None, _native.loss_photo_backward(*ctx.saved_tensors, g_value, *ctx.cfg), None, None, None, None


class _DcFn(torch.autograd.Function):
    """depth_consistency under autograd: (value, count)."""

    @staticmethod
    def forward(ctx, large, small):
        ctx.set_materialize_grads(False)
        value, count = _native.loss_dc(large, small)
        ctx.save_for_backward(large, small, count)
        ctx.mark_non_differentiable(count)
        return value, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_count):
        want_large, want_small = ctx.needs_input_grad
        if g_value is None or not (want_large or want_small):
            return None, None
        return _native.loss_dc_backward(*ctx.saved_tensors, g_value, want_large=want_large, want_small=want_small)


class _SmoothFn(torch.autograd.Function):
    """edge_aware_smoothness under autograd."""

    @staticmethod
    def forward(ctx, depth, rgb):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(depth, rgb)
        return _native.loss_smooth(depth, rgb)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value):
        if g_value is None or not ctx.needs_input_grad[0]:
            return None, None
        return _native.loss_smooth_backward(*ctx.saved_tensors, g_value), None


class _Smooth1Fn(torch.autograd.Function):
    """smooth_grad_1st under autograd."""

    @staticmethod
    def forward(ctx, flo, image, alpha):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(flo, image)
        ctx.alpha = alpha
        return _native.loss_smooth1(flo, image, alpha)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value):
        if g_value is None or not ctx.needs_input_grad[0]:
            return None, None, None
        flo, image = ctx.saved_tensors
        return _native.loss_smooth1_backward(flo, image, ctx.alpha, g_value), None, None


class _FlowWarpFn(torch.autograd.Function):
    """flow_warp under autograd: the forward is the no-grad kernel call; the backward asks the kernels only for the gradients that
    are needed."""

    @staticmethod
    def forward(ctx, x, flow, pad, deterministic):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, flow)
        ctx.cfg = (pad, deterministic)
        return _native.flow_warp(x, flow, pad)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        want_x, want_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_out is None or not (want_x or want_flow):
            return None, None, None, None
        x, flow = ctx.saved_tensors
        pad, deterministic = ctx.cfg
        g_x, g_f = _native.flow_warp_backward(x, flow, g_out, pad, want_x=want_x, want_flow=want_flow, deterministic=deterministic)
        return g_x, g_f, None, None


class _FlowPhotoFn(torch.autograd.Function):
    """flow_photometric under autograd: (value, count); the backward recomputes from the inputs."""

    @staticmethod
    def forward(ctx, im, other, flow, mask, w_l1, w_ssim, w_ternary, pad):
        ctx.set_materialize_grads(False)
        ctx.cfg = (w_l1, w_ssim, w_ternary, pad)
        value, count = _native.flow_photo(im, other, flow, mask, *ctx.cfg)
        ctx.save_for_backward(im, other, flow, mask, count)
        ctx.mark_non_differentiable(count)
        return value, count

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_count):
        if g_value is None or not ctx.needs_input_grad[2]:
            return (None,) * 8
        return None, None, _native.flow_photo_backward(*ctx.saved_tensors, g_value, *ctx.cfg), None, None, None, None, None


class _FlowCostVolumeFn(torch.autograd.Function):
    """flow_cost_volume under autograd: the forward is the no-grad kernel call and saves its own result (the activation's factor is
    read from it); the backward asks the kernels only for the gradients that are needed."""

    @staticmethod
    def forward(ctx, x1, x2, flow, max_displacement, negative_slope, pad, deterministic):
        ctx.set_materialize_grads(False)
        out = _native.flow_cost_volume(x1, x2, flow, max_displacement, negative_slope, pad)
        ctx.has_flow = flow is not None
        ctx.save_for_backward(*((x1, x2, flow, out) if ctx.has_flow else (x1, x2, out)))
        ctx.cfg = (max_displacement, negative_slope, pad, deterministic)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        want1, want2, wantf = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_flow and ctx.needs_input_grad[2]
        if g_out is None or not (want1 or want2 or wantf):
            return (None,) * 7
        saved = ctx.saved_tensors
        x1, x2, flow, out = saved if ctx.has_flow else (saved[0], saved[1], None, saved[2])
        md, slope, pad, deterministic = ctx.cfg
        g1, g2, gf = _native.flow_cost_volume_backward(x1, x2, flow, out, g_out, md, slope, pad, want_x1=want1, want_x2=want2,
                                                       want_flow=wantf, deterministic=deterministic)
        return g1, g2, gf, None, None, None, None


class _SsimFn(torch.autograd.Function):
    """ssim under autograd."""

    @staticmethod
    def forward(ctx, x, y, md):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, y)
        ctx.md = md
        return _native.ssim(x, y, md)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_out is None or not (want_x or want_y):
            return None, None, None
        x, y = ctx.saved_tensors
        g_x, g_y = _native.ssim_backward(x, y, g_out, ctx.md, want_x=want_x, want_y=want_y)
        return (g_x.to(x.dtype) if want_x else None), (g_y.to(y.dtype) if want_y else None), None


class _TernaryFn(torch.autograd.Function):
    """ternary under autograd."""

    @staticmethod
    def forward(ctx, x, y, md):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, y)
        ctx.md = md
        return _native.ternary(x, y, md)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_out is None or not (want_x or want_y):
            return None, None, None
        x, y = ctx.saved_tensors
        g_x, g_y = _native.ternary_backward(x, y, g_out, ctx.md, want_x=want_x, want_y=want_y)
        return (g_x.to(x.dtype) if want_x else None), (g_y.to(y.dtype) if want_y else None), None


class _CorrelationFn(torch.autograd.Function):
    """Autograd binding like models/correlation_package/correlation.py:6-44 (CorrelationFunction)."""

    @staticmethod
    def forward(ctx, x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply):
        ctx.save_for_backward(x1, x2)
        ctx.cfg = (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
        return _native.correlation_forward(x1, x2, *ctx.cfg)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x1, x2 = ctx.saved_tensors
        g1, g2 = _native.correlation_backward(x1, x2, grad_out, *ctx.cfg, want1=ctx.needs_input_grad[0],
                                              want2=ctx.needs_input_grad[1])
        return g1, g2, None, None, None, None, None, None


def correlation(x1, x2, pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1):
    """The reference's native correlation op, forward and backward (models/correlation_package/correlation.py:6-61)."""
    if x1.requires_grad or x2.requires_grad:
        return _CorrelationFn.apply(x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
    return _native.correlation_forward(x1, x2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
