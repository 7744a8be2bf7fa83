"""The yardstick of the fused consistency and smoothness terms (csrc/loss_terms.hip): a float64 restatement of the four terms of
losses/loss_blocks.py in plain torch -- inverse_warp and transform_dmap restated too, gradients by float64 autograd -- and the
maker of the inputs the per-term tests use.  The restatement takes the float32 inputs and the float32 Kinv / proj the kernels
get and promotes them; it imports nothing from oracle/ or from the package.

The maker builds inputs on which float32 and float64 must take the same decisions (taps, masks, minima), and asserts it on the
CPU in float64, so that no pixel has to be left out of a comparison."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 1e-3
# (B, H, W) -> the small map of the down-sample term is [B, H // 4, W // 4] (none for H < 4)
SHAPES = ((2, 36, 48), (3, 17, 23), (1, 4, 4), (1, 2, 2), (2, 64, 96))


# ---- float64 restatement -----------------------------------------------------------------------------------------------------------
def _lower(B, H, W):
    keep = torch.ones(B, H, W, dtype=torch.bool)
    keep[:, 0:int(H / 3)] = False
    return keep


def positions64(depth, Kinv, proj):
    """Normalised and un-normalised sample positions of inverse_warp (pixel2cam, cam2pixel, grid_sample align_corners=False):
    (xn, yn, ix, iy), each [B,H,W] float64, differentiable with respect to depth."""
    B, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(1, 3, H * W)
    cam = torch.matmul(Kinv.double(), pix) * depth.double().reshape(B, 1, H * W)
    pc = torch.matmul(proj.double()[:, :, :3], cam) + proj.double()[:, :, 3:]
    Z = pc[:, 2].clamp(min=FLOOR)
    xn = 2 * (pc[:, 0] / Z) / (W - 1) - 1
    yn = 2 * (pc[:, 1] / Z) / (H - 1) - 1
    ix = ((xn + 1) * W - 1) / 2
    iy = ((yn + 1) * H - 1) / 2
    return tuple(t.reshape(B, H, W) for t in (xn, yn, ix, iy))


def warp64(img, depth, Kinv, proj, mode):
    """inverse_warp in float64: (warped [B,C,H,W], valid bool [B,H,W])."""
    xn, yn, _, _ = positions64(depth, Kinv, proj)
    warped = F.grid_sample(img.double(), torch.stack([xn, yn], dim=-1), mode=mode, padding_mode="zeros", align_corners=False)
    return warped, (torch.maximum(xn.abs(), yn.abs()) <= 1).detach()


def moved64(src_depth, pose_row, intr):
    """transform_dmap in float64: the z of every source pixel's point in the target camera (pose_row: third row of the pose)."""
    B, H, W = src_depth.shape
    K, P = intr.double(), pose_row.double().expand(B, 4)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xs = (xs - K[:, 0, 2, None, None]) / K[:, 0, 0, None, None]
    ys = (ys - K[:, 1, 2, None, None]) / K[:, 1, 1, None, None]
    z = src_depth.double().clamp(min=FLOOR)
    c = [P[:, i, None, None] for i in range(4)]
    return c[0] * (xs * z) + c[1] * (ys * z) + c[2] * z + c[3]


def _rel(a, b):
    return ((a - b).abs() / (a + b).abs()).clamp(0, 1)


def _per_item(x):
    return x.reshape(x.shape[0], -1).sum(1)


def dsc64(src_depth, tgt_depth, src_mask, Kinv, proj, pose_row, intr):
    """-> (value [B], count [B]) in float64."""
    B, H, W = tgt_depth.shape
    moved = moved64(src_depth, pose_row, intr) * src_mask.double().reshape(B, H, W)
    warped, valid = warp64(moved.unsqueeze(1), tgt_depth, Kinv, proj, "nearest")
    warped = warped[:, 0]
    m = (valid & _lower(B, H, W) & (warped > 0)).double()
    tgt = (tgt_depth.double() * m).clamp(min=FLOOR)
    got = (warped * m).clamp(min=FLOOR)
    return _per_item(_rel(tgt, got) * m) / _per_item(m), _per_item(m)


def rsc64(src_rgb, tgt_rgb, tgt_depth, Kinv, proj):
    B, H, W = tgt_depth.shape
    warped, valid = warp64(src_rgb, tgt_depth, Kinv, proj, "bilinear")
    m = (valid & _lower(B, H, W)).double().unsqueeze(1)
    diff = (tgt_rgb.double() * m - warped * m).abs()
    return _per_item(diff * m) / (3 * _per_item(m)), _per_item(m)


def dc64(large, small):
    B, h, w = small.shape
    keep = _lower(B, h, w).double()
    pooled = (-F.max_pool2d(-large.double().unsqueeze(1), 4)).squeeze(1).clamp(min=FLOOR)
    s = small.double().clamp(min=FLOOR)
    return _per_item(_rel(pooled, s) * keep) / _per_item(keep), _per_item(keep)


def smooth64(depth, rgb):
    d, im = depth.double().unsqueeze(1), rgb.double()
    rows = (d[:, :, :-1] - d[:, :, 1:]).abs() * torch.exp(-(im[:, :, :-1] - im[:, :, 1:]).abs().mean(1, keepdim=True))
    cols = (d[:, :, :, :-1] - d[:, :, :, 1:]).abs() * torch.exp(-(im[:, :, :, :-1] - im[:, :, :, 1:]).abs().mean(1, keepdim=True))
    return rows.mean((1, 2, 3)) + cols.mean((1, 2, 3))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def intrinsics(B, H, W):
    """The camera of util_loss.py (fx 41, fy 40, centre (24.3, 17.6) on 36 x 48), scaled to H x W."""
    K = np.array([[41.0 * W / 48, 0.0, 24.3 * W / 48], [0.0, 40.0 * H / 36, 17.6 * H / 36], [0.0, 0.0, 1.0]])
    return torch.from_numpy(np.tile(K, (B, 1, 1)).astype(np.float32))


def stereo_pose():
    """Target-to-source pose: a 0.54 m baseline and a small rotation about the vertical axis ([4,4] float32).  The vertical
    offset (5 cm) outweighs what the rotation does to the rows, so that the first and the last row -- which the reference's
    normalisation by H - 1 puts half a pixel outside the image, on the rounding boundary of the nearest tap -- stay on one side of
    it whatever the depth; along x the positions are decided by the depth, pixel by pixel."""
    a = 0.002
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T[:3, 3] = [-0.54, 0.05, 0.0]
    return torch.from_numpy(T.astype(np.float32))


def _smooth_depth(rs, B, H, W):
    """8 to 36 m, smooth (a coarse grid blown up bilinearly) plus 0.5 m of noise."""
    coarse = torch.from_numpy(9.0 + 26.0 * rs.rand(B, 1, max(H // 8, 2), max(W // 8, 2)))
    return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[:, 0]


def _noise(rs, shape):
    return torch.from_numpy(rs.rand(*shape) - 0.5)


def _trouble(tgt, K, T):
    """Pixels [B,H,W] of the target depth map whose decisions float32 and float64 might take differently."""
    B, H, W = tgt.shape
    Kd = K.double()
    xn, yn, ix, iy = positions64(tgt, torch.inverse(Kd), torch.matmul(Kd, T.double()[None, :3]).expand(B, 3, 4))
    bad = torch.zeros(B, H, W, dtype=torch.bool)
    for p in (ix, iy):
        frac = p - p.floor()
        bad |= (frac - 0.5).abs() < 1e-3                       # the rounding boundary of the nearest tap
        bad |= torch.minimum(frac, 1 - frac) < 1e-4            # the cell boundary of the bilinear taps (its gradient jumps there)
    for p in (xn, yn):
        bad |= (p.abs() - 1).abs() < 1e-5                      # the boundary of `valid`
    if H >= 4 and W >= 4:                                      # two depths of a 4x4 block within 1e-5 relative of each other
        h, w = H // 4, W // 4
        blk = tgt[:, :4 * h, :4 * w].reshape(B, h, 4, w, 4).permute(0, 1, 3, 2, 4).reshape(B, h, w, 16)
        order = blk.argsort(-1)
        srt = blk.gather(-1, order)
        close = (srt[..., 1:] - srt[..., :-1]) < 1e-5 * srt[..., 1:]
        hit = torch.zeros_like(blk, dtype=torch.bool).scatter(-1, order[..., 1:], close)
        bad[:, :4 * h, :4 * w] |= hit.reshape(B, h, w, 4, 4).permute(0, 1, 3, 2, 4).reshape(B, 4 * h, 4 * w)
    return bad


def make_inputs(B, H, W, seed=100):
    """-> dict of float32 CPU tensors: src_depth, tgt_depth [B,H,W] (the target is also the large map of the down-sample term),
    src_mask [B,H,W] at 50 % (all ones on maps of at most 16 pixels), small [B,H//4,W//4] (None for H < 4), src_rgb, tgt_rgb [B,3,H,W], intr [B,3,3], T [4,4] (target to
    source).  The seed advances -- for the pixels in trouble only: a pixel's position depends on its own depth alone -- until, in
    float64 on the CPU, no sample position lies within 1e-3 px of a rounding boundary of the nearest tap (or 1e-4 px of a cell
    boundary of the bilinear taps), no |xn|, |yn| within 1e-5 of 1, no warped depth within 1e-3 of 0 and no two depths of a 4x4
    block within 1e-5 relative of each other; all of it is asserted on what is returned."""
    rs = np.random.RandomState(seed + 7919 * (H * W + B))
    K, T = intrinsics(B, H, W), stereo_pose()
    base = _smooth_depth(rs, B, H, W)
    tgt = (base + _noise(rs, base.shape)).float()
    for _ in range(200):
        bad = _trouble(tgt, K, T)
        if not bool(bad.any()):
            break
        tgt = torch.where(bad, (base + _noise(rs, base.shape)).float(), tgt)
    src = (_smooth_depth(rs, B, H, W) + _noise(rs, base.shape)).float()
    mask = torch.from_numpy((rs.rand(B, H, W) < 0.5).astype(np.float32))
    if H * W <= 16:   # (the few pixels of such a map that land inside the source must count)
        mask = torch.ones_like(mask)
    out = {"tgt_depth": tgt, "src_depth": src, "src_mask": mask, "intr": K, "T": T, "small": None}
    if H >= 4 and W >= 4:
        pooled = -F.max_pool2d(-tgt.unsqueeze(1), 4)[:, 0]
        out["small"] = (pooled * torch.from_numpy(1.0 + 0.2 * (rs.rand(*pooled.shape) - 0.5))).float()
    for name in ("src_rgb", "tgt_rgb"):
        coarse = torch.from_numpy(rs.randn(B, 3, H // 4 + 1, W // 4 + 1))
        up = coarse.repeat_interleave(4, 2).repeat_interleave(4, 3)[..., :H, :W]
        out[name] = (up + 0.1 * torch.from_numpy(rs.randn(B, 3, H, W))).float()
    # the four conditions, on what is returned
    assert not bool(_trouble(out["tgt_depth"], K, T).any()), (B, H, W)
    moved = moved64(src, torch.inverse(T.double())[None, 2], K)
    assert float(moved.abs().min()) > 1e-3
    assert float(out["tgt_depth"].min()) > 1.0 and float(out["src_depth"].min()) > 1.0
    return out


def camera_matrices(intr, T, inv3):
    """(Kinv [B,3,3], proj [B,3,4], back [1,4,4]) in float32 where intr lives, formed as BaseLoss forms them: inv3 =
    loss_blocks._inv3, proj = intr @ T[:3]; back = the inverse pose (inverted on the host in float32), whose third row back[:, 2]
    the depth-stereo term takes."""
    B = intr.shape[0]
    pose = T.unsqueeze(0).to(intr.device)
    back = torch.inverse(T).unsqueeze(0).to(intr.device)
    return inv3(intr).expand(B, 3, 3).contiguous(), torch.matmul(intr, pose[:, 0:3, :]).expand(B, 3, 4).contiguous(), back
