"""The photometric term of one direction of the unsupervised flow loss restated in float64, and the seeded inputs of its tests
(tests/test_flow_photo_host.py, tests/test_flow_photo_gpu.py; csrc/flow_photo.hip, ops.flow_photometric).

  photo64            value of one direction: util_flow.flow_warp_ref, then the masked L1 mean, util_ssim.ssim_dist and
                     util_ternary.ternary_dist of the masked images, over the mean of the mask -- the nested `photo` of
                     util_flow.unflow_ref, lifted out, with the warp inside; in the dtype of its inputs, differentiable by autograd
  unflow_via_photo64 util_flow.unflow_ref with photo64 in the place of its nested function: the four values
  make_inputs        im, other (util_flow.smooth_image), a smooth flow of a few pixels with the plants of util_flow._plants on a
                     handful of pixels, a 0 / 1 mask with about a fifth zeros in blobs; float32 numpy, and the planted pixels
  left_out           the share of unplanted pixels the gradient comparison leaves out (util_flow.near_jump), and the kept pixels
"""
import types

import numpy as np
import torch
import torch.nn.functional as F

import util_flow as U
import util_occlusion as UO
import util_ssim as US
import util_ternary as UT

# (B, h, w): one window and one interior census pixel; the fixture's coarsest level; a partial tile; three tiles across and three
# down (64 x 8 pixels a tile), so halos cross tile edges in both axes; more than one item of more than one tile
SHAPES = ((1, 3, 3), (2, 6, 10), (2, 19, 27), (1, 17, 130), (2, 33, 66))
WEIGHTS = ((0.15, 0.85, 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
PADS = U.PADS
LEFT_OUT_CAP = 0.01   # at most this share of the unplanted pixels may be left out of the gradient comparison
SEED = 3100


def cfg_of(weights, pad="border"):
    """The attributes unFlowLoss.loss_photomatric reads."""
    return types.SimpleNamespace(w_l1=weights[0], w_ssim=weights[1], w_ternary=weights[2], warp_pad=pad)


def photo64(im, other, flow, mask, weights, pad):
    w_l1, w_ssim, w_ternary = weights
    recons = U.flow_warp_ref(other, flow, pad)
    total = 0
    if w_l1 > 0:
        total = total + (w_l1 * (im - recons).abs() * mask).mean()
    if w_ssim > 0:
        total = total + (w_ssim * US.ssim_dist(recons * mask, im * mask, 1)).mean()
    if w_ternary > 0:
        total = total + (w_ternary * UT.ternary_dist(recons * mask, im * mask, 1)).mean()
    # (a mask is float32 in the reference and in the package whatever the images are: its mean, count / n, is rounded to float32)
    return total / mask.float().mean()


def unflow_via_photo64(cfg, flows, target):
    """(total, warp, smooth, mean |flow|) as util_flow.unflow_ref sums them, every direction's photometric term from photo64."""
    images = (target[:, :3], target[:, 3:])
    weights = (cfg.w_l1, cfg.w_ssim, cfg.w_ternary)
    first, warp_terms, smooth_terms, s = None, [], [], 1.0
    for i, flow in enumerate(flows):
        if cfg.w_scales[i] == 0:
            warp_terms.append(0)
            smooth_terms.append(0)
            continue
        B, _, h, w = flow.shape
        fwd, bwd = flow[:, :2], flow[:, 2:]
        im1, im2 = (F.interpolate(im, (h, w), mode="area") for im in images)
        if i == 0:
            masks = []
            for a, b in ((fwd.detach(), bwd.detach()), (bwd.detach(), fwd.detach())):
                if cfg.occ_from_back:
                    r = UO.range_map(UO.base_grid(B, h, w, dtype=b.dtype) + b).clamp(0, 1)
                    masks.append(1 - (r < 0.2).to(flow.dtype))
                else:
                    masks.append(1 - U.fb_check_ref(a, b)[0].to(flow.dtype))
            first, s = masks, min(h, w)
        else:
            masks = [F.interpolate(m, (h, w), mode="nearest") for m in first]
        warp = photo64(im1, im2, fwd, masks[0], weights, cfg.warp_pad)
        smooth = U.smooth_ref(fwd / s, im1, cfg.alpha)
        if cfg.with_bk:
            warp = (warp + photo64(im2, im1, bwd, masks[1], weights, cfg.warp_pad)) / 2
            smooth = (smooth + U.smooth_ref(bwd / s, im2, cfg.alpha)) / 2
        warp_terms.append(warp * cfg.w_scales[i])
        smooth_terms.append(smooth * cfg.w_sm_scales[i])
    warp_loss, smooth_loss = sum(warp_terms), cfg.w_smooth * sum(smooth_terms)
    return warp_loss + smooth_loss, warp_loss, smooth_loss, flows[0].abs().mean()


def make_inputs(shape):
    """-> {im, other [B,3,h,w], flow [B,2,h,w], mask [B,1,h,w], planted [B,h,w] bool}, numpy.  The flow is 2.5 px times a bilinear
    upsampling of N(0, 1) on a 4 x 5 grid; planted on top, at pixels spread over the batch (at most every second pixel, the most
    important plants first): exact integer positions, positions exactly at 0 and at w - 1 / h - 1 and one representable position
    either side, positions leaving the image on each side, a flow of +-1e6.  The mask is 0 where a smooth noise field is below its
    own 20 % quantile: blobs."""
    B, h, w = shape
    seed = SEED + 10 * SHAPES.index(tuple(shape))
    rs = np.random.RandomState(seed)
    im, other = U.smooth_image(B, h, w, seed + 1), U.smooth_image(B, h, w, seed + 2)
    flow = (2.5 * U._upsampled_noise(rs, B, 2, h, w)).numpy().astype(np.float32)
    field = U._upsampled_noise(rs, B, 1, h, w, 3, 4).numpy()
    mask = (field > np.quantile(field, 0.2)).astype(np.float32)
    plants = U._plants(h, w)
    n = min(len(plants), (B * h * w) // 2)
    planted = np.zeros((B, h, w), bool)
    for k, at in enumerate(np.linspace(0, B * h * w - 1, n).astype(int)):
        b, rem = divmod(int(at), h * w)
        y, xx = divmod(rem, w)
        planted[b, y, xx] = True
        for axis, (what, base, size) in enumerate(((plants[k][0], xx, w), (plants[k][1], y, h))):
            if what is None:
                continue
            if what[0] == "flow":
                flow[b, axis, y, xx] = what[1]
            else:
                t = (base + 3 + k) % size if what[1] == "int" else what[1]
                flow[b, axis, y, xx] = U._aim(base, size, t, what[2])
    out = {"im": im, "other": other, "flow": flow, "mask": mask, "planted": planted}
    for pad in PADS:   # the inputs stay within the cap: a seed that breaks it is changed
        share, _ = left_out(out, pad)
        assert share <= LEFT_OUT_CAP, (shape, pad, share)
    return out


def left_out(inputs, pad):
    """-> (share of the unplanted pixels whose own float64 position is near a jump of d R / d flow, keep [B,h,w] bool)."""
    jump = U.near_jump(torch.from_numpy(inputs["flow"]).double(), pad)
    free = ~torch.from_numpy(inputs["planted"])
    return float(jump[free].double().mean()), ~jump
