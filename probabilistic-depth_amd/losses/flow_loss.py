"""The unsupervised optical-flow loss with the name and interface of the reference's losses/flow_loss.py:8-118, so that code
written against it imports unchanged: unFlowLoss(cfg)(output, target) -> (total, warp_loss, smooth_loss, mean |flow|).

What a scale composes, in the order of the reference's loss_photomatric (:13-27):
    warps                  ops.flow_warp (csrc/flow_warp.hip; differentiable in the flow, an order-independent scatter under
                           torch.use_deterministic_algorithms)
    first-scale masks      1 - get_occu_mask_backward on the range-map op (csrc/occlusion.hip) when cfg.occ_from_back, else
                           1 - ops.flow_fb_check; constants, as the reference's .float() of a comparison
    coarser-scale masks    nearest interpolation of the first scale's
    photometric pieces     |a - b| m, ops.ssim and ops.ternary on the masked images, each a mean, their sum over mean(m)
    smoothness             ops.smooth_grad_1st(flow / s, image, alpha), s = min(h, w) of the first scale
The 'area' resizes of the images stay F.interpolate.  Device fp32 tensors only: the ops have no CPU path.  Nothing is printed and
nothing is read back to the host.

unFlowLoss(cfg, fused_photo=True): the warp and the photometric pieces of a scale and direction are one ops.flow_photometric call
(csrc/flow_photo.hip: three launches for forward and backward together); the masks, the resizes and the smoothness are the ones
above.  Off by default; off, every output bit is the composition's.

cfg attributes: w_l1, w_ssim, w_ternary, alpha, warp_pad, occ_from_back, with_bk, w_scales, w_sm_scales, w_smooth.
"""
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils.warp_utils import get_occu_mask_backward


class _Switches(type):
    """unFlowLoss(cfg, fused_photo=False): the switch is taken at the call of the class, so that __init__ keeps the reference's
    signature -- cfg alone -- for code that subclasses or inspects it."""

    def __call__(cls, cfg, fused_photo=False):
        loss = super().__call__(cfg)
        loss.fused_photo = bool(fused_photo)
        return loss


class unFlowLoss(nn.Module, metaclass=_Switches):
    fused_photo = False

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg

    def loss_photomatric(self, im1_scaled, im1_recons, occu_mask1):
        """The weighted photometric pieces of one direction, each averaged, over the mean of the visibility mask."""
        cfg = self.cfg
        seen, recons = im1_scaled * occu_mask1, im1_recons * occu_mask1
        total = 0
        if cfg.w_l1 > 0:
            total = total + (cfg.w_l1 * (im1_scaled - im1_recons).abs() * occu_mask1).mean()
        if cfg.w_ssim > 0:
            total = total + (cfg.w_ssim * ops.ssim(recons, seen)).mean()
        if cfg.w_ternary > 0:
            total = total + (cfg.w_ternary * ops.ternary(recons, seen)).mean()
        return total / occu_mask1.mean()

    def _photometric(self, im, other, flow, mask):
        """The photometric term of one direction: `other` warped along `flow` against `im` under `mask`."""
        cfg = self.cfg
        if self.fused_photo:
            return ops.flow_photometric(im, other, flow, mask, cfg.w_l1, cfg.w_ssim, cfg.w_ternary, pad=cfg.warp_pad)[0]
        return self.loss_photomatric(im, ops.flow_warp(other, flow, pad=cfg.warp_pad), mask)

    def loss_smooth(self, flow, im1_scaled):
        return ops.smooth_grad_1st(flow, im1_scaled, self.cfg.alpha)

    def _first_masks(self, fwd, bwd):
        """Visibility masks (1 = seen) of the two images at the first scale; the flows enter detached: a mask is a constant."""
        fwd, bwd = fwd.detach(), bwd.detach()
        if self.cfg.occ_from_back:
            return 1 - get_occu_mask_backward(bwd, th=0.2), 1 - get_occu_mask_backward(fwd, th=0.2)
        return 1 - ops.flow_fb_check(fwd, bwd), 1 - ops.flow_fb_check(bwd, fwd)

    def forward(self, output, target):
        """output: the multi-scale flows, n x [B,4,h,w] (channels 0:2 the flow 1 -> 2, 2:4 the flow 2 -> 1), finest first;
        target: the image pair [B,6,H,W].  -> total, warp loss, smoothness loss, mean |flow| of the finest scale."""
        cfg = self.cfg
        images = (target[:, :3], target[:, 3:])
        self.pyramid_occu_mask1, self.pyramid_occu_mask2 = [], []
        warp_terms, smooth_terms = [], []
        s = 1.
        for i, flow in enumerate(output):
            if cfg.w_scales[i] == 0:
                warp_terms.append(0)
                smooth_terms.append(0)
                continue
            h, w = flow.shape[2:]
            fwd, bwd = flow[:, :2], flow[:, 2:]
            im1, im2 = (F.interpolate(im, (h, w), mode='area') for im in images)
            if i == 0:
                mask1, mask2 = self._first_masks(fwd, bwd)
                s = min(h, w)
            else:
                mask1 = F.interpolate(self.pyramid_occu_mask1[0], (h, w), mode='nearest')
                mask2 = F.interpolate(self.pyramid_occu_mask2[0], (h, w), mode='nearest')
            self.pyramid_occu_mask1.append(mask1)
            self.pyramid_occu_mask2.append(mask2)

            warp = self._photometric(im1, im2, fwd, mask1)
            smooth = self.loss_smooth(fwd / s, im1)
            if cfg.with_bk:
                warp = (warp + self._photometric(im2, im1, bwd, mask2)) / 2.
                smooth = (smooth + self.loss_smooth(bwd / s, im2)) / 2.
            warp_terms.append(warp * cfg.w_scales[i])
            smooth_terms.append(smooth * cfg.w_sm_scales[i])

        warp_loss = sum(warp_terms)
        smooth_loss = cfg.w_smooth * sum(smooth_terms)
        return warp_loss + smooth_loss, warp_loss, smooth_loss, output[0].abs().mean()
