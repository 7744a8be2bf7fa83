"""The terms of the training loss, with the names and argument lists of the reference's losses/loss_blocks.py so that code
written against it imports unchanged.  Every function takes the reference's single-item shapes and also a batch; with
per_item=True the masked means are taken per batch item and returned as a [B] vector (the reference calls these functions
once per item and adds the results, losses/losses.py:90-194).

Nothing here reads a value back to the host.  The warps are the HIP inverse_warp of utils/inverse_warp.py ('nearest' for
depth, 'bilinear' for RGB); the 3x3 intrinsics are inverted in closed form on the device (torch.inverse checks its status
on the host).
"""
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import img_utils
from ..utils import inverse_warp as iv


def _sum_hw(x, per_item):
    return x.reshape(x.shape[0], -1).sum(1) if per_item else x.sum()


def mean_on_mask(diff, valid_mask, per_item=False):
    """sum(diff * mask) / sum(mask), the mask broadcast over diff (loss_blocks.py:68-71)."""
    mask = valid_mask.expand_as(diff)
    return _sum_hw(diff * mask, per_item) / _sum_hw(mask, per_item)


def _lower_two_thirds(shape, device):
    """1 below the top third of the rows ([B,H,W]): the part of the image the consistency terms look at."""
    keep = torch.ones(shape, dtype=torch.bool, device=device)
    keep[:, 0:int(shape[1] / 3), :] = False
    return keep


def _visibility(occlusion, shape):
    """An occlusion= argument, [B,1,H,W] | [B,H,W], as the fp32 [B,1,H,W] factor of a term's mask of that shape."""
    vis = occlusion.float()
    vis = vis.unsqueeze(1) if vis.dim() == 3 else vis
    if tuple(vis.shape) != tuple(shape):
        raise RuntimeError(f"occlusion must be {list(shape)} or {[shape[0]] + list(shape[2:])}, got {list(occlusion.shape)}")
    return vis


def _inv3(m):
    """Inverse of [B,3,3] matrices by the adjugate: elementwise, on the device the matrices live on."""
    a, b, c, d, e, f, g, h, i = m.reshape(-1, 9).unbind(1)
    co = torch.stack([e * i - f * h, c * h - b * i, b * f - c * e,
                      f * g - d * i, a * i - c * g, c * d - a * f,
                      d * h - e * g, b * g - a * h, a * e - b * d], dim=1)
    det = a * co[:, 0] + b * co[:, 3] + c * co[:, 6]
    return (co / det[:, None]).reshape(m.shape)


def _inv4(pose):
    """Inverse of a 4x4 pose where it lives: on the CPU by torch.inverse, on the device without the host-side status check."""
    return torch.linalg.inv_ex(pose).inverse if pose.is_cuda else torch.inverse(pose)


def _warp(img, depth, pose, intr, mode):
    """iv.inverse_warp for [B,4,4] | [1,4,4] poses, from matrices formed without a host check."""
    B = img.shape[0]
    intr = intr.float()
    proj = torch.matmul(intr, pose[:, 0:3, :].float()).expand(B, 3, 4)
    return iv.warp_with_matrices(img, depth, _inv3(intr).expand(B, 3, 3), proj, mode)


def soft_cross_entropy_loss(soft_label, x, mask=None, BV_log=False, d_candi=None):
    """-sum_d label * log p, averaged over the pixels whose mask is 1 (loss_blocks.py:186-202): soft_label, x [B,D,H,W],
    mask [B,H,W] | [B,1,H,W] | None.  One fused HIP pass (ops.dpv_soft_ce).  With B == 1 the scalar the reference returns
    (0 for a mask without a valid pixel, decided on the device: a tensor, never the float 0.); with B > 1 the [B] vector."""
    logp = x if BV_log else F.log_softmax(x, dim=1)
    dc = d_candi if d_candi is not None else torch.zeros(logp.shape[1], dtype=torch.float32, device=logp.device)
    loss, _ = ops.dpv_soft_ce(logp, dc, label=soft_label, mask=mask)
    return loss[0] if loss.shape[0] == 1 else loss


def edge_aware_smoothness_loss(pred_disp, img, max_scales):
    """First-order smoothness of each map in pred_disp ([B,1,h,w]), down-weighted across image edges, the scales weighted
    1, 1/4, 1/16 ... (loss_blocks.py:73-112)."""
    def diff_rows(t):
        return t[:, :, :-1, :] - t[:, :, 1:, :]

    def diff_cols(t):
        return t[:, :, :, :-1] - t[:, :, :, 1:]

    loss, weight = 0, 1.0
    for disp in pred_disp[:max_scales]:
        scaled = F.adaptive_avg_pool2d(img, disp.shape[2:])
        w_rows = torch.exp(-diff_rows(scaled).abs().mean(1, keepdim=True))
        w_cols = torch.exp(-diff_cols(scaled).abs().mean(1, keepdim=True))
        loss = loss + ((diff_rows(disp).abs() * w_rows).mean() + (diff_cols(disp).abs() * w_cols).mean()) * weight
        weight /= 4.0
    return loss


def SSIM(x, y, md=1):
    """clamp((1 - SSIM(x, y)) / 2, 0, 1) over (2 md + 1)^2 windows, [B,C,H,W] -> [B,C,H-2md,W-2md] (loss_blocks.py:47-66): one HIP
    pass forward, one backward (ops.ssim; md = 1, 2 or 3)."""
    return ops.ssim(x, y, md)


def TernaryLoss(im, im_warp, max_distance=1):
    """Ternary census distance of two RGB images over (2 max_distance + 1)^2 patches, [B,3,H,W] -> [B,1,H,W], 0 within max_distance
    of a border (loss_blocks.py:8-44): one HIP pass forward, one backward (ops.ternary; max_distance = 1, 2 or 3)."""
    return ops.ternary(im, im_warp, max_distance)


def gradient(data):
    """Forward differences (D_dx [..., W-1], D_dy [..., H-1, :]) of a [B,C,H,W] tensor (loss_blocks.py:204-207); plain slicing."""
    D_dy = data[:, :, 1:] - data[:, :, :-1]
    D_dx = data[:, :, :, 1:] - data[:, :, :, :-1]
    return D_dx, D_dy


def smooth_grad_1st(flo, image, alpha):
    """Edge-aware first-order smoothness of a flow [B,Cf,H,W] under an image [B,Ci,H,W] of the same size (loss_blocks.py:210-220):
    one HIP pass forward, one backward with respect to flo (ops.smooth_grad_1st); a 0-dim tensor."""
    return ops.smooth_grad_1st(flo, image, alpha)


def rgb_stereo_consistency_loss(src_rgb_img, target_rgb_img, target_depth_map, pose_target2src, intr, viz=False, per_item=False,
                                occlusion=None, ternary_weight=0.0, ternary_md=1, ssim_weight=0.0, ssim_md=1, fused=False):
    """Photometric error between the target image and the source image warped into it with the target's depth map, over the
    pixels that land inside the source and lie below the top third (loss_blocks.py:114-145).  rgb [B,3,H,W], depth [B,H,W],
    pose [1,4,4] | [B,4,4], intr [B,3,3].  viz is accepted and ignored (the reference opens a window).

    ssim_weight = w != 0 mixes in the SSIM distance the reference carries commented out (loss_blocks.py:128-129, where it suggests
    0.85), composed as its flow loss composes the photometric pieces (losses/flow_loss.py:13-27): with m the mask,
        (1 - w) mean_on_mask(|tgt m - warped m|, m) + w mean(SSIM(warped m, tgt m, ssim_md)) / mean(m),
    the means per item with per_item.  With w == 0 the SSIM is not evaluated: the L1 term alone, with the bits it has always had.

    fused=True with w != 0: the same term as one HIP pass each way (ops.rgb_stereo_consistency, csrc/photo.hip) instead of the
    composition below; the [B] vector with per_item, else the value of the single item (B == 1: the batch mean of the composition
    and the item's mean are then one thing).  With w == 0 fused changes nothing.

    ternary_weight = wt != 0 mixes in the third piece of that flow loss, the census distance, the same way: with ws = ssim_weight,
        (1 - ws - wt) L1 + ws mean(SSIM) / mean(m) + wt mean(TernaryLoss(warped m, tgt m, ternary_md)) / mean(m),
    a piece whose weight is 0 not evaluated.  With wt == 0 the op is not called and the path, and so the bits, are those above.
    The single-pass op has no census term: fused=True with wt != 0 is a RuntimeError.

    occlusion: a visibility map of the target view, [B,1,H,W] | [B,H,W], 1 where some source pixel sees the target pixel
    (ops.depth_occlusion of the source's depth map; the occu_mask of losses/flow_loss.py:72-78).  It multiplies the mask m before
    anything is averaged, so the band beside a depth edge that the source camera cannot see is left out of every piece.  With None
    not one operation changes.  The single-pass op has no mask input: fused=True with an occlusion map is a RuntimeError."""
    if fused and occlusion is not None:
        raise RuntimeError("rgb_stereo_consistency_loss: fused=True is the single-pass op (csrc/photo.hip), which has no mask input; "
                           "an occlusion map needs fused=False")
    if fused and ternary_weight != 0:
        raise RuntimeError("rgb_stereo_consistency_loss: fused=True is the single-pass op (csrc/photo.hip), which has no census term; "
                           f"ternary_weight={ternary_weight} needs fused=False")
    if fused and ssim_weight != 0:
        B = src_rgb_img.shape[0]
        if not per_item and B != 1:
            raise RuntimeError("rgb_stereo_consistency_loss: fused=True returns per-item values; pass per_item=True for a batch "
                               f"(B={B}), or one item at a time")
        intr = intr.float()
        proj = torch.matmul(intr, pose_target2src[:, 0:3, :].float()).expand(B, 3, 4)
        value, _ = ops.rgb_stereo_consistency(src_rgb_img, target_rgb_img, target_depth_map, _inv3(intr).expand(B, 3, 3), proj,
                                              ssim_weight=ssim_weight, ssim_md=ssim_md)
        return value if per_item else value[0]
    warped, valid = _warp(src_rgb_img, target_depth_map, pose_target2src, intr, "bilinear")
    mask = (valid & _lower_two_thirds(valid.shape, src_rgb_img.device)).float().unsqueeze(1)
    if occlusion is not None:
        mask = mask * _visibility(occlusion, mask.shape)
    diff = (target_rgb_img * mask - warped * mask).abs()
    photo = mean_on_mask(diff, mask, per_item)
    if ssim_weight == 0 and ternary_weight == 0:
        return photo

    def over_mask(dist):
        if per_item:
            return dist.reshape(dist.shape[0], -1).mean(1) / mask.reshape(mask.shape[0], -1).mean(1)
        return dist.mean() / mask.mean()

    total = (1.0 - ssim_weight - ternary_weight) * photo   # (wt == 0: the factor, and the operations below, are those of the SSIM mix alone)
    if ssim_weight != 0:
        total = total + ssim_weight * over_mask(SSIM(warped * mask, target_rgb_img * mask, ssim_md))
    if ternary_weight != 0:
        total = total + ternary_weight * over_mask(TernaryLoss(warped * mask, target_rgb_img * mask, ternary_md))
    return total


def depth_stereo_consistency_loss(src_depth_img, target_depth_img, src_depth_mask, target_depth_mask, pose_target2src, intr,
                                  pose_src2target=None, per_item=False, occlusion=None):
    """Relative difference between the target depth map and the source depth map brought into the target view: the source
    depths are re-expressed in the target camera (transform_dmap with the inverse pose), masked, and fetched with a nearest
    warp along the target's own depth (loss_blocks.py:147-171).  depth maps [B,1,H,W], masks [B,1,H,W] | [B,H,W], pose
    [1,4,4] | [B,4,4], intr [B,3,3].  pose_src2target: the inverse of the pose where the caller already has it (else it is
    inverted here); target_depth_mask is unused, as in the reference.  occlusion: a visibility map of the target view as
    rgb_stereo_consistency_loss takes it; it multiplies the term's mask before the average.  With None not one operation changes."""
    B, _, H, W = src_depth_img.shape
    back = pose_src2target if pose_src2target is not None else _inv4(pose_target2src)
    moved = iv.transform_dmap(src_depth_img[:, 0], back, intr)
    moved = (moved * src_depth_mask.float().reshape(B, H, W)).unsqueeze(1)
    warped, valid = _warp(moved, target_depth_img[:, 0], pose_target2src, intr, "nearest")
    mask = (valid & _lower_two_thirds(valid.shape, src_depth_img.device)).unsqueeze(1) & (warped > 0.)
    mask = mask.float()
    if occlusion is not None:
        mask = mask * _visibility(occlusion, mask.shape)
    tgt = (target_depth_img * mask).clamp(min=1e-3)
    got = (warped * mask).clamp(min=1e-3)
    diff = ((tgt - got).abs() / (tgt + got).abs()).clamp(0, 1)
    return mean_on_mask(diff, mask, per_item)


def depth_consistency_loss(large_dm, small_dm, per_item=False):
    """Relative difference between the low-resolution depth map and the 4x4 minimum of the full-resolution one, below the
    top third (loss_blocks.py:173-184).  large_dm [B,H,W], small_dm [B,H/4,W/4]."""
    keep = _lower_two_thirds(small_dm.shape, large_dm.device).float()
    pooled = img_utils.minpool(large_dm.unsqueeze(1), 4).squeeze(1).clamp(min=1e-3)
    small = small_dm.clamp(min=1e-3)
    diff = ((pooled - small).abs() / (pooled + small).abs()).clamp(0, 1)
    return mean_on_mask(diff, keep, per_item)
