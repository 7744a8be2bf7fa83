"""The yardstick of the fused photometric term (csrc/photo.hip; ops.rgb_stereo_consistency with ssim_weight != 0): a float64
restatement in plain torch from the pieces the merged suites already pin -- the warp and the L1 term of util_loss_terms.py, the
SSIM of util_ssim.py --, gradients by float64 autograd, and the maker of the inputs the tests use.  It imports nothing from
oracle/ or from the package.

The maker builds inputs on which float32 and float64 must take the same decisions: the depth, pose and intrinsics are
util_loss_terms.make_inputs' (taps, masks), and the images are drawn so that no window's (1 - S) / 2 lies within util_ssim.EDGE
of a clamp edge without being exactly on it.  Both are asserted on the CPU in float64, so that no window and no pixel has to
be left out of a comparison."""
import numpy as np
import torch
import torch.nn.functional as F

import util_loss_terms as LT
import util_ssim as U

W_SSIM = 0.85
# (B, H, W): two shapes of util_loss_terms.SHAPES; the tile width (64) and one either side of it, one row past the tile height
# (16); three tile rows; three tile columns with one spare pixel; one window at md = 3; one window at md = 1 (two valid pixels)
SHAPES = ((2, 36, 48), (3, 17, 23), (1, 17, 63), (1, 17, 64), (1, 17, 65), (2, 33, 66), (2, 18, 129), (1, 7, 7), (1, 3, 3))
CASES = [(shape, md) for shape in SHAPES for md in U.MDS if min(shape[1:]) >= 2 * md + 1]


# ---- float64 restatement -----------------------------------------------------------------------------------------------------------
def pieces64(src, tgt, depth, Kinv, proj, md):
    """-> (l1 [B], structural [B], count [B]) in float64: the masked L1 mean, mean(SSIM(warped m, tgt m)) / mean(m), sum(m)."""
    B, H, W = depth.shape
    warped, valid = LT.warp64(src, depth, Kinv, proj, "bilinear")
    m = (valid & LT._lower(B, H, W)).double().unsqueeze(1)
    count = LT._per_item(m)
    diff = (tgt.double() * m - warped * m).abs()
    l1 = LT._per_item(diff * m) / (3 * count)
    dist = U.ssim_parts(warped * m, tgt.double() * m, md)["raw"].clamp(0, 1)
    structural = dist.reshape(B, -1).mean(1) / m.reshape(B, -1).mean(1)
    return l1, structural, count


def photo64(src, tgt, depth, Kinv, proj, w, md):
    """-> (value [B], count [B]) in float64: (1 - w) L1 + w SSIM / mean(mask) per item; differentiable with respect to depth."""
    l1, structural, count = pieces64(src, tgt, depth, Kinv, proj, md)
    return (1 - w) * l1 + w * structural, count


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _images(rs, B, H, W):
    """(src, tgt) [B,3,H,W] float32 in [0, 1] that share their coarse structure; the source's noise is drawn first."""
    coarse = torch.from_numpy(rs.uniform(0, 1, (B, 3, max(H // 4, 2), max(W // 4, 2))))
    base = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    src = 0.8 * base + 0.2 * torch.from_numpy(rs.uniform(0, 1, (B, 3, H, W)))
    tgt = 0.8 * base + 0.2 * torch.from_numpy(rs.uniform(0, 1, (B, 3, H, W)))
    return src.float(), tgt.float()


def matrices64(inp):
    """(Kinv, proj) in float64 from the maker's intrinsics and pose (the tests form the float32 ones on the device)."""
    K = inp["intr"].double()
    return torch.inverse(K), torch.matmul(K, inp["T"].double()[None, :3]).expand(K.shape[0], 3, 4)


def check_inputs(inp, md):
    """The maker's two conditions, in float64 on the CPU: -> (windows near a clamp edge without being on it, smallest count)."""
    Kinv, proj = matrices64(inp)
    B, H, W = inp["tgt_depth"].shape
    warped, valid = LT.warp64(inp["src_rgb"], inp["tgt_depth"], Kinv, proj, "bilinear")
    m = (valid & LT._lower(B, H, W)).double().unsqueeze(1)
    raw = U.ssim_parts(warped * m, inp["tgt_rgb"].double() * m, md)["raw"]
    return int(U.near_edge(raw).sum()), float(LT._per_item(m).min())


def make_inputs(B, H, W, md):
    """util_loss_terms.make_inputs(B, H, W) with the images replaced: dict of float32 CPU tensors (tgt_depth [B,H,W], src_rgb,
    tgt_rgb [B,3,H,W], intr [B,3,3], T [4,4] target to source, ...).  The image seed advances until no window is near a clamp edge
    and every item has a pixel in its mask; both are asserted on what is returned."""
    out = dict(LT.make_inputs(B, H, W))
    for bump in range(50):
        rs = np.random.RandomState(9100 + H * W + md + 7919 * bump)
        out["src_rgb"], out["tgt_rgb"] = _images(rs, B, H, W)
        near, least = check_inputs(out, md)
        if near == 0 and least > 0:
            break
    near, least = check_inputs(out, md)
    assert near == 0 and least > 0, (B, H, W, md, near, least)
    return out
