"""Golden fixture g23: gradients of the reference's training chain with respect to the feature maps and the volumes.  Build
container only (imports the reference, which never travels):

    python tests/golden/make_golden_bwd.py

  * est_swp_volume_v4 (warping/homography.py:98-135) for L2 and L1 at V = 2 (view 1 sends part of the image out of bounds,
    like g3), with a seeded upstream gradient of the cost volume: the cost and feat_img_ref.grad / feat_img_src.grad;
  * the PacknetModel chain log_softmax -> dpv_to_depthmap(BV_log=True) (models/packnet.py:394, utils/img_utils.py:52-61)
    and dpv_to_depthmap(BV_log=False), each with a seeded upstream gradient of the depth map and the input's gradient.
C = 11, D = 16, 24 x 32.  Nothing of the reference is copied: its functions are imported and called.  Data only.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference, _cam_dict, _rays_and_K, _rot  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    homo, view, img_utils = _import_reference()
    torch.manual_seed(23)
    h, w, C, D, V = 24, 32, 11, 16, 2
    rays, K = _rays_and_K(view, w, h, 80.0, 35.0)
    K[0, 2] += 1.3
    K[1, 2] -= 0.7
    cam = _cam_dict(K, rays)
    d_candi = img_utils.powerf(5.0, 40.0, D, 1.0)
    ref = torch.randn(1, C, h, w)
    src = torch.randn(1, V, C, h, w)
    R = torch.from_numpy(np.stack([_rot(0.02, -0.01, 0.005), _rot(0.4, 0.0)]).astype(np.float32))
    t = torch.from_numpy(np.array([[0.3, 0.02, 0.1], [0.0, -9.0, 0.5]], dtype=np.float32))
    K32 = cam["intrinsic_M_cuda"]
    out = dict(ref=ref.numpy(), src=src.numpy(), K=K32.numpy()[None], R=R.numpy()[None], t=t.numpy()[None],
               rays=rays.numpy()[None], cxcy=np.array([[K32[0, 2], K32[1, 2]]], dtype=np.float32), d_candi=d_candi,
               sigma=np.float32(10.0))
    for metric in ("L2", "L1"):
        r, s = ref.clone().requires_grad_(True), src.clone().requires_grad_(True)
        cost = homo.est_swp_volume_v4(r, s, d_candi, R, t, cam, 10.0, feat_dist=metric)
        gcost = torch.randn(cost.shape)
        (cost * gcost).sum().backward()
        out.update({metric + "_cost": cost.detach().numpy(), metric + "_gcost": gcost.numpy(), metric + "_gref": r.grad.numpy(),
                    metric + "_gsrc": s.grad.numpy()})
    for tag, bv_log in (("lsm", True), ("plain", False)):
        x = (3 * torch.randn(1, D, h, w)).requires_grad_(True)
        y = F.log_softmax(x, dim=1) if bv_log else x
        depth = img_utils.dpv_to_depthmap(y, d_candi, BV_log=bv_log)
        gdepth = torch.randn(depth.shape)
        (depth * gdepth).sum().backward()
        out.update({tag + "_in": x.detach().numpy(), tag + "_gdepth": gdepth.numpy(), tag + "_grad": x.grad.numpy()})
    np.savez_compressed(os.path.join(HERE, "g23_sweep_backward.npz"), **out)


if __name__ == "__main__":
    main()
