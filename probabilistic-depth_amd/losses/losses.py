"""BaseLoss / DefaultLoss with the signature, the target keys and the weighting of the reference's losses/losses.py.

BaseLoss.forward(output, target): output = (left, right) dicts with "output" / "output_refined" (lists of log-DPVs
[B,D,h,w] / [B,D,H,W]); target = (left, right) dicts with soft_labels, soft_labels_imgsize (lists of [D,h,w] or tensors
[B,D,h,w]), masks, masks_imgsizes [B,1,h,w], intrinsics, intrinsics_up [B,3,3], rgb [B,V,3,H,W], T_left2right [4,4],
d_candi; cfg.loss.{ce,dsc,dc,rsc,rsc_low,smooth}_mul.

Against the reference: every volume goes through ONE ops.dpv_soft_ce call for the whole batch (the reference walks items
and sides in Python, losses.py:32-67), the depth maps of the last volumes come out of the same pass (the reference
regresses them again, :80-88), an item without a valid pixel contributes 0 on the device, and nothing is read back to the
host: no .item(), no truth test on a tensor, no host copy.  With labels_from_depth=True and dmaps / dmap_imgsizes in the
target, the soft labels are formed inside the kernel from the depth maps (variance cfg.var.softce, prepared as the loader
does: clamp(d_candi[0], d_candi[-1]) * mask, kittiloader/batch_scheduler.py:105-106) and soft_labels* may be absent.

With fused_terms=True the consistency and smoothness terms (dc, dsc, rsc, smooth) are the fused HIP passes of csrc/loss_terms.hip
(ops.depth_consistency, depth_stereo_consistency, rgb_stereo_consistency, edge_aware_smoothness) instead of the torch compositions
of loss_blocks.py.  The camera matrices they take are formed with the helpers the compositions use (_inv3, intr @ pose[:3]), once
per (intrinsics, pose) pair of the call, so the masks keep their bits.  The default is the composition.

cfg.loss.rsc_ssim = w (absent: 0) mixes the SSIM distance into the two RGB consistency terms, rsc and rsc_low, over windows of half-width
cfg.loss.rsc_ssim_md (absent: 1): (1 - w) L1 + w SSIM / mean(mask) per item, loss_blocks.rgb_stereo_consistency_loss; the reference's
commented-out line (loss_blocks.py:128-129) suggests 0.85.  With fused_terms=True alone and w != 0 the rsc term stays the composition
(the HIP warp and the HIP SSIM, ops.ssim), the other fused terms stay fused.  With the key absent or 0 no path changes.

With fused_photo=True and w != 0 both RGB terms, rsc and rsc_low, are the single-pass photometric op instead (csrc/photo.hip,
ops.rgb_stereo_consistency(..., ssim_weight=w, ssim_md=md): warp, L1 and SSIM in one launch each way), whatever fused_terms says;
the low-resolution images still come from F.interpolate, the camera matrices from the helper the fused terms use.  With the key
absent or 0, fused_photo changes nothing.  The default is False.

cfg.loss.rsc_ternary = wt (absent: 0) mixes the ternary census distance (ops.ternary, csrc/ternary.hip) into the same two terms,
over patches of half-width cfg.loss.rsc_ternary_md (absent: 1): (1 - w - wt) L1 + w SSIM / mean(mask) + wt census / mean(mask)
per item.  The fused passes have no census term, so with wt != 0 both terms are the composition of
loss_blocks.rgb_stereo_consistency_loss around the HIP warp and the HIP ops, whatever fused_terms and fused_photo say; the other
fused terms stay fused.  With the key absent or 0 no path changes.

cfg.loss.occ != 0 (absent: 0) leaves the pixels that the other camera cannot see out of the rsc, rsc_low and dsc terms.  Per call
four visibility masks are computed, two sides at two resolutions, by splatting the other side's depth map into the view
(ops.depth_occlusion, csrc/occlusion.hip; threshold cfg.loss.occ_th, absent: 0.2) with the camera pair of the term of the opposite
direction, which the call caches anyway: the mask describes the warp that term performs.  The masks are constants (no gradient
reaches a depth map through them) and order-independent sums: the same bits from call to call.  The fused passes have no mask
input, so with occ != 0 those three terms are the compositions of loss_blocks (occlusion=...), whatever fused_terms and
fused_photo say; the other fused terms stay fused.  With the key absent or 0 no path changes.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .loss_blocks import (_inv3, depth_consistency_loss, depth_stereo_consistency_loss, edge_aware_smoothness_loss,
                          rgb_stereo_consistency_loss)


def _stacked(labels):
    return labels if isinstance(labels, torch.Tensor) else torch.stack(list(labels))


class BaseLoss(nn.Module):
    def __init__(self, cfg, id, labels_from_depth=False, fused_terms=False, fused_photo=False):
        super().__init__()
        self.cfg = cfg
        self.id = id
        self.labels_from_depth = labels_from_depth
        self.fused_terms = fused_terms
        self.fused_photo = fused_photo

    def _cross_entropy(self, volumes, tgt, label_key, depth_key, mask_key, d_candi):
        """(sum over the volumes and the items of the per-item cross-entropy, depth map [B,h,w] of the last volume)."""
        mask = tgt[mask_key][:, 0]
        src = {}
        if self.labels_from_depth and depth_key in tgt:
            src["depth_gt"] = tgt[depth_key].float().clamp(float(d_candi[0]), float(d_candi[-1])) * mask
            src["variance"] = float(self.cfg.var.softce)
        else:
            src["label"] = _stacked(tgt[label_key])
        total, depth = 0, None
        for n, vol in enumerate(volumes):
            loss, dm = ops.dpv_soft_ce(vol, d_candi, mask=mask, want_depth=(n == len(volumes) - 1), **src)
            total = total + loss.sum()
            depth = dm if dm is not None else depth
        return total, depth

    def forward(self, output, target):
        # fp32 throughout, also when called inside a torch.autocast region: the log-DPVs arrive in fp32, and autocast would hand
        # the camera products below to the fp32-only kernels in half precision
        with torch.autocast(output[0]["output"][-1].device.type, enabled=False):
            return self._forward(output, target)

    def _forward(self, output, target):
        out_l, out_r = output
        tgt_l, tgt_r = target
        mul = self.cfg.loss
        device = out_l["output"][-1].device
        d_candi = tgt_l["d_candi"]
        B = out_l["output"][-1].shape[0]

        # cross-entropy of every volume; the depth maps of the last low-resolution and refined volumes
        ce_loss, ce_count = 0, 0
        small, large = {}, {}
        for side, out, tgt in (("l", out_l, tgt_l), ("r", out_r, tgt_r)):
            lo, small[side] = self._cross_entropy(out["output"], tgt, "soft_labels", "dmaps", "masks", d_candi)
            hi, large[side] = self._cross_entropy(out["output_refined"], tgt, "soft_labels_imgsize", "dmap_imgsizes",
                                                  "masks_imgsizes", d_candi)
            ce_loss = ce_loss + lo + hi
        ce_count = (len(out_l["output"]) + len(out_l["output_refined"])) * B   # (left and right of an item count once)

        # the pose between the two cameras and its inverse, inverted where it arrives (a CPU tensor from the loader)
        T = tgt_l["T_left2right"].float()
        T_inv = torch.inverse(T) if not T.is_cuda else torch.linalg.inv_ex(T).inverse
        pose_l2r = T.unsqueeze(0).to(device, non_blocking=True)     # target = left, source = right
        pose_r2l = T_inv.unsqueeze(0).to(device, non_blocking=True)

        fused = self.fused_terms
        cams = {}

        def camera(intr, pose):
            """(Kinv [B,3,3], proj [B,3,4]) of an (intrinsics, pose) pair as loss_blocks._warp forms them, once per call."""
            key = (id(intr), id(pose))
            if key not in cams:
                k = intr.float()
                cams[key] = (_inv3(k).expand(B, 3, 3), torch.matmul(k, pose[:, 0:3, :].float()).expand(B, 3, 4))
            return cams[key]

        dc_loss = 0
        if mul.dc_mul != 0 and fused:
            dc_loss = (ops.depth_consistency(large["l"], small["l"])[0].sum() +
                       ops.depth_consistency(large["r"], small["r"])[0].sum())
        elif mul.dc_mul != 0:
            dc_loss = (depth_consistency_loss(large["l"], small["l"], per_item=True).sum() +
                       depth_consistency_loss(large["r"], small["r"], per_item=True).sum())

        # visibility of each view from the other one, per resolution: {} with cfg.loss.occ absent or 0
        occ = getattr(mul, "occ", 0) != 0
        occ_th = getattr(mul, "occ_th", 0.2)
        seen = {}

        def visible(hi):
            """{"l", "r"} -> {"occlusion": visible [B,1,h,w]} of the view that is the term's target, once per resolution."""
            if not occ:
                return {"l": {}, "r": {}}
            if hi not in seen:
                dm = large if hi else small
                ik = "intrinsics_up" if hi else "intrinsics"
                seen[hi] = {"l": {"occlusion": ops.depth_occlusion(dm["r"], *camera(tgt_r[ik], pose_r2l), th=occ_th)},
                            "r": {"occlusion": ops.depth_occlusion(dm["l"], *camera(tgt_l[ik], pose_l2r), th=occ_th)}}
            return seen[hi]

        dsc_loss = 0
        if mul.dsc_mul != 0:
            for hi in (True, False):
                dm = large if hi else small
                mk = "masks_imgsizes" if hi else "masks"
                ik = "intrinsics_up" if hi else "intrinsics"
                if fused and not occ:   # right into left, then left into right
                    Kinv, proj = camera(tgt_l[ik], pose_l2r)
                    dsc_loss = dsc_loss + ops.depth_stereo_consistency(dm["r"], dm["l"], tgt_r[mk], Kinv, proj, pose_r2l[:, 2],
                                                                       tgt_l[ik].float())[0].sum()
                    Kinv, proj = camera(tgt_r[ik], pose_r2l)
                    dsc_loss = dsc_loss + ops.depth_stereo_consistency(dm["l"], dm["r"], tgt_l[mk], Kinv, proj, pose_l2r[:, 2],
                                                                       tgt_r[ik].float())[0].sum()
                    continue
                dl, dr = dm["l"].unsqueeze(1), dm["r"].unsqueeze(1)
                # right into left, then left into right
                vis = visible(hi)
                dsc_loss = dsc_loss + depth_stereo_consistency_loss(dr, dl, tgt_r[mk], tgt_l[mk], pose_l2r, tgt_l[ik],
                                                                    pose_src2target=pose_r2l, per_item=True, **vis["l"]).sum()
                dsc_loss = dsc_loss + depth_stereo_consistency_loss(dl, dr, tgt_l[mk], tgt_r[mk], pose_r2l, tgt_r[ik],
                                                                    pose_src2target=pose_l2r, per_item=True, **vis["r"]).sum()

        rgb_l, rgb_r = tgt_l["rgb"][:, -1], tgt_r["rgb"][:, -1]
        ssim_w, ssim_md = getattr(mul, "rsc_ssim", 0.0), getattr(mul, "rsc_ssim_md", 1)
        photo = {"ssim_weight": ssim_w, "ssim_md": ssim_md} if ssim_w != 0 else {}
        census_w = getattr(mul, "rsc_ternary", 0.0)
        if census_w != 0:
            photo.update(ternary_weight=census_w, ternary_md=getattr(mul, "rsc_ternary_md", 1))
        one_pass = self.fused_photo and ssim_w != 0 and census_w == 0 and not occ

        def photometric(src, tgt, depth, intr, pose):
            return ops.rgb_stereo_consistency(src, tgt, depth, *camera(intr, pose), **photo)[0].sum()

        rsc_loss = 0
        if mul.rsc_mul != 0 and one_pass:
            rsc_loss = (photometric(rgb_r, rgb_l, large["l"], tgt_l["intrinsics_up"], pose_l2r) +
                        photometric(rgb_l, rgb_r, large["r"], tgt_r["intrinsics_up"], pose_r2l))
        elif mul.rsc_mul != 0 and fused and ssim_w == 0 and census_w == 0 and not occ:
            rsc_loss = (ops.rgb_stereo_consistency(rgb_r, rgb_l, large["l"], *camera(tgt_l["intrinsics_up"], pose_l2r))[0].sum() +
                        ops.rgb_stereo_consistency(rgb_l, rgb_r, large["r"], *camera(tgt_r["intrinsics_up"], pose_r2l))[0].sum())
        elif mul.rsc_mul != 0:
            vis = visible(True)
            rsc_loss = (rgb_stereo_consistency_loss(rgb_r, rgb_l, large["l"], pose_l2r, tgt_l["intrinsics_up"], per_item=True, **photo,
                                                    **vis["l"]).sum() +
                        rgb_stereo_consistency_loss(rgb_l, rgb_r, large["r"], pose_r2l, tgt_r["intrinsics_up"], per_item=True, **photo,
                                                    **vis["r"]).sum())

        rsc_low_loss = 0
        if mul.rsc_low_mul != 0:
            low_l = F.interpolate(rgb_l, scale_factor=0.25, mode="bilinear")
            low_r = F.interpolate(rgb_r, scale_factor=0.25, mode="bilinear")
        if mul.rsc_low_mul != 0 and one_pass:
            rsc_low_loss = (photometric(low_r, low_l, small["l"], tgt_l["intrinsics"], pose_l2r) +
                            photometric(low_l, low_r, small["r"], tgt_r["intrinsics"], pose_r2l))
        elif mul.rsc_low_mul != 0:
            vis = visible(False)
            rsc_low_loss = (rgb_stereo_consistency_loss(low_r, low_l, small["l"], pose_l2r, tgt_l["intrinsics"], per_item=True, **photo,
                                                        **vis["l"]).sum() +
                            rgb_stereo_consistency_loss(low_l, low_r, small["r"], pose_r2l, tgt_r["intrinsics"], per_item=True, **photo,
                                                        **vis["r"]).sum())

        smooth_loss = 0
        if mul.smooth_mul != 0 and fused:
            smooth_loss = ops.edge_aware_smoothness(large["l"], rgb_l).sum() + ops.edge_aware_smoothness(large["r"], rgb_r).sum()
        elif mul.smooth_mul != 0:   # (a mean over the batch times B = the sum of the per-item means)
            smooth_loss = B * (edge_aware_smoothness_loss([large["l"].unsqueeze(1)], rgb_l, 1) +
                               edge_aware_smoothness_loss([large["r"].unsqueeze(1)], rgb_r, 1))

        loss = torch.zeros((), dtype=torch.float32, device=device)
        bsize = float(2 * B)
        if bsize != 0:
            loss = loss + ((ce_loss / ce_count) * mul.ce_mul + (dsc_loss / bsize) * mul.dsc_mul + (dc_loss / bsize) * mul.dc_mul +
                           (rsc_loss / bsize) * mul.rsc_mul + (rsc_low_loss / bsize) * mul.rsc_low_mul +
                           (smooth_loss / bsize) * mul.smooth_mul)
        return loss


class DefaultLoss(nn.Module):
    """The placeholder of the reference (losses/losses.py:212-239): the L1 norm of the last low-resolution volumes of both
    sides, once per item of the batch."""

    def __init__(self, cfg, id):
        super().__init__()
        self.cfg = cfg
        self.id = id

    def forward(self, output, target):
        out_l, out_r = output
        n = len(target[0]["soft_labels"])
        return n * (out_l["output"][-1].abs().sum() + out_r["output"][-1].abs().sum())
