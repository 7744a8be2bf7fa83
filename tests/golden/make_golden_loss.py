"""Golden fixture g24: the reference's training loss.  Build container only (imports the reference, which never travels):

    python tests/golden/make_golden_loss.py

Inputs: tests/util_loss.py (D = 16, B = 2, 9 x 12 and 36 x 48, left / right; rebuilt by the tests from the same frozen random
streams -- the fixture stores their checksums).  Stored, all from the reference's own functions on the CPU:
  * gen_soft_label_torch(zero_invalid=True) labels of the low-resolution depth maps (utils/img_utils.py:31-47);
  * soft_cross_entropy_loss(BV_log=True) and x.grad per item of the low-resolution volumes, with the fixture's masks and with
    an all-zero mask (losses/loss_blocks.py:186-202: the float 0., no gradient);
  * transform_dmap (utils/inverse_warp.py:212-253), minpool with and without a default (utils/img_utils.py:87-95), and each
    term of losses/loss_blocks.py on item 0;
  * BaseLoss.forward of the whole structure with the multipliers of configs/default_mono.json and the gradients with respect
    to the four volumes (losses/losses.py:14-210).
One item of the structure (left, item 1, low resolution) has a mask without an entry equal to one (0.5 where valid): its
cross-entropy is 0 and it counts in ce_count.  (A mask that is zero everywhere would make the reference's stereo term of that
item 0 / 0: that case is in the per-item cross-entropy data only.)
Checked here: no ground-truth depth lies between 7 and 9 m beyond the last candidate (there the label would depend on how an
exp implementation flushes to zero); the float32 reference against its own float64 run differs, in the volume gradients, at
no more than 0.1 % of the pixels (nearest-neighbour taps and clamps that flip).  Data only; nothing of the reference is copied.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util_loss as U  # noqa: E402


def _run_base(ref_losses, ref_iv, img_utils, inp, dtype):
    ref_iv.pixel_coords = None   # (the reference caches its pixel grid in the dtype of the first call)
    output, target = U.structure(inp, img_utils.gen_soft_label_torch, dtype=dtype)
    loss = ref_losses.BaseLoss(U.loss_cfg(), 0)(output, target)
    loss.backward()
    return loss.detach(), [v.grad.detach() for v in U.volumes(output)]


def main():
    _, _, img_utils = _import_reference()
    import losses.loss_blocks as lb
    import losses.losses as ref_losses
    import utils.inverse_warp as ref_iv
    inp = U.make_inputs()
    dc = U.d_candi()
    for k, v in inp.items():
        if k.startswith("dmap"):
            beyond = v - dc[-1]
            assert not ((beyond > 7.0) & (beyond < 9.0)).any(), k
    out = dict(U.checksums(inp))
    out["d_candi"] = np.asarray(dc)
    # labels, per-item cross-entropy
    for s in U.SIDES:
        labels = U.soft_labels(inp, img_utils.gen_soft_label_torch, s, "lo")
        out[f"label_{s}_lo"] = torch.stack(labels).numpy()
        for i in range(U.B):
            for tag, mask in (("", torch.from_numpy(inp[f"mask_{s}_lo"][i])), ("_zero", torch.zeros(1, *U.LO))):
                x = torch.from_numpy(inp[f"logp_{s}_lo"][i:i + 1]).requires_grad_(True)
                l = lb.soft_cross_entropy_loss(labels[i].unsqueeze(0), x, mask=mask, BV_log=True)
                if isinstance(l, torch.Tensor):
                    l.backward()
                    out[f"ce{tag}_{s}_{i}"], out[f"ce{tag}_grad_{s}_{i}"] = l.detach().numpy(), x.grad.numpy()
                else:
                    out[f"ce{tag}_{s}_{i}"], out[f"ce{tag}_grad_{s}_{i}"] = np.float32(l), np.zeros_like(inp[f"logp_{s}_lo"][i:i + 1])
    # blocks on item 0
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    T, Tinv = t["T_left2right"], torch.inverse(t["T_left2right"])
    out["transform_dmap"] = ref_iv.transform_dmap(t["dmap_left_hi"][0], Tinv, t["K_hi"][0]).numpy()
    sparse = t["dmap_left_hi"] * t["mask_left_hi"][:, 0]
    out["minpool"] = img_utils.minpool(t["dmap_left_hi"].unsqueeze(0), 4).numpy()
    out["minpool_default"] = img_utils.minpool(sparse.unsqueeze(0), 4, 1000).numpy()
    dl, dr = t["dmap_left_hi"][0:1], t["dmap_right_hi"][0:1].clamp(max=40.0)
    ref_iv.pixel_coords = None
    out["blk_dc"] = lb.depth_consistency_loss(dl, t["dmap_left_lo"][0:1]).numpy()
    out["blk_dsc"] = lb.depth_stereo_consistency_loss(dr.unsqueeze(0), dl.unsqueeze(0), t["mask_right_hi"][0], t["mask_left_hi"][0],
                                                      T.unsqueeze(0), t["K_hi"][0:1]).numpy()
    out["blk_rsc"] = lb.rgb_stereo_consistency_loss(t["rgb_right"][0:1, 0], t["rgb_left"][0:1, 0], dl, T.unsqueeze(0), t["K_hi"][0:1]).numpy()
    out["blk_smooth"] = lb.edge_aware_smoothness_loss([dl.unsqueeze(0)], t["rgb_left"][0:1, 0], 1).numpy()
    out["blk_mean_on_mask"] = lb.mean_on_mask(t["rgb_left"][0:1, 0], t["mask_left_hi"][0:1]).numpy()
    # the whole loss, float32 and float64
    loss, grads = _run_base(ref_losses, ref_iv, img_utils, inp, torch.float32)
    loss64, grads64 = _run_base(ref_losses, ref_iv, img_utils, inp, torch.float64)
    assert torch.isfinite(loss) and abs(float(loss) - float(loss64)) <= 1e-5 * abs(float(loss64)), (float(loss), float(loss64))
    for g, g64 in zip(grads, grads64):
        per_pixel = (g.double() - g64).abs().amax(1)
        share = float((per_pixel > 1e-3 * g64.abs().max()).double().mean())
        assert share <= 1e-3, share
    out["base_loss"] = loss.numpy()
    out["base_loss64"] = loss64.numpy()
    for name, g in zip(("left_lo", "left_hi", "right_lo", "right_hi"), grads):
        out["base_grad_" + name] = g.numpy()
    path = os.path.join(HERE, "g24_loss.npz")
    np.savez_compressed(path, **out)
    print("base loss", float(loss), float(loss64), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
