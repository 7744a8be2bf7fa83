"""The range map and the occlusion mask restated from their definition, for the tests of ops.range_map, ops.occlusion_mask and
ops.depth_occlusion (tests/test_occlusion_host.py, tests/test_occlusion_gpu.py), the fixture maker
(tests/golden/make_golden_occlusion.py) and the baseline of tools/bench_occlusion.py.

  range_map          the splat, in the dtype and on the device of its positions: float64 = the tests' reference, float32 on the
                     device = "the torch composition" the bench times; want_count: also the number of contributions per destination
  visible            the mask of a range map: 0 where clamp(r, 0, 1) < th
  depth_positions    the depth-to-position chain in the formulas of utils/inverse_warp.py:26-69 (pixel2cam, cam2pixel) plus the
                     align_corners=False un-normalisation, in the dtype of the depth map
  base_grid          pixel coordinates [B,2,H,W]
  scene / flows      the seeded inputs of the fixture's cases;  analytic_band: the mask of the two-disparity flow, by construction
  cases              tests/golden/g27_occlusion.npz by case name
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g27_occlusion.npz")
THS = (0.2, 0.5)
MARGIN = 1e-3          # no pixel of a case has clamp(r, 0, 1) this close to a threshold (asserted by the maker, in float64)
DEPTH_CASES = ("a", "b", "c", "d")
FLOW_CASES = ("e_int", "e_quarter", "e_collide", "e_edge", "e_nonfinite")
COLLIDE_AT = (5, 9)    # (x, y) every pixel of e_collide is aimed at
BAND = dict(d_bg=1, d_fg=4, rows=(4, 11), cols=(6, 12))   # e_int: the box of disparity d_fg on a background of disparity d_bg


def base_grid(B, H, W, dtype=torch.float32, device="cpu"):
    ys = torch.arange(H, dtype=dtype, device=device).view(1, 1, H, 1).expand(B, 1, H, W)
    xs = torch.arange(W, dtype=dtype, device=device).view(1, 1, 1, W).expand(B, 1, H, W)
    return torch.cat((xs, ys), 1).contiguous()


def range_map(coords, want_count=False):
    """coords [B,2,H,W] -> r [B,1,H,W] (, count [B,1,H,W]): every source pixel adds (1 - |dx|)(1 - |dy|) to the four pixels around its
    position, the in-bounds ones only; a non-finite position adds nothing.  No value is read back to the host."""
    B, _, H, W = coords.shape
    x, y = coords[:, 0].reshape(B, -1), coords[:, 1].reshape(B, -1)
    finite = torch.isfinite(x) & torch.isfinite(y)
    x, y = torch.where(finite, x, torch.full_like(x, -8.0)), torch.where(finite, y, torch.full_like(y, -8.0))
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    r = torch.zeros(B, H * W, dtype=coords.dtype, device=coords.device)
    n = torch.zeros_like(r)
    for dx, wx in ((0, 1 - fx), (1, fx)):
        for dy, wy in ((0, 1 - fy), (1, fy)):
            tx, ty = x0 + dx, y0 + dy
            inside = finite & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
            at = (ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)).long()
            r.scatter_add_(1, at, torch.where(inside, wx * wy, torch.zeros_like(wx)))
            if want_count:
                n.scatter_add_(1, at, inside.to(coords.dtype))
    r = r.view(B, 1, H, W)
    return (r, n.view(B, 1, H, W)) if want_count else r


def visible(r, th):
    """1 where some source pixel sees the pixel: not (clamp(r, 0, 1) < th), as float32."""
    return 1.0 - (r.clamp(0.0, 1.0) < th).float()


def margin(r):
    """The least distance of clamp(r, 0, 1) from a threshold of THS."""
    c = r.double().clamp(0.0, 1.0)
    return min(float((c - th).abs().min()) for th in THS)


def depth_positions(depth, Kinv, proj):
    """depth [B,H,W], Kinv [B,3,3], proj [B,3,4] -> un-normalised positions [B,2,H,W] of the source pixels in the other view:
    cam = (Kinv (x, y, 1)) d;  p = proj[:, :, :3] cam + proj[:, :, 3];  Z = max(p_z, 1e-3);
    xn = 2 (p_x / Z) / (W - 1) - 1, yn likewise with H;  ix = ((xn + 1) W - 1) / 2, iy = ((yn + 1) H - 1) / 2."""
    B, H, W = depth.shape
    grid = base_grid(B, H, W, depth.dtype, depth.device)
    pix = torch.cat((grid, torch.ones_like(grid[:, :1])), 1).reshape(B, 3, -1)
    cam = torch.matmul(Kinv, pix) * depth.reshape(B, 1, -1)
    p = torch.matmul(proj[:, :, :3], cam) + proj[:, :, 3:]
    Z = p[:, 2].clamp(min=1e-3)
    xn = 2 * (p[:, 0] / Z) / (W - 1) - 1
    yn = 2 * (p[:, 1] / Z) / (H - 1) - 1
    ix = ((xn + 1) * W - 1) / 2
    iy = ((yn + 1) * H - 1) / 2
    return torch.stack((ix, iy), 1).reshape(B, 2, H, W)


# ---- the fixture's inputs -----------------------------------------------------------------------------------------------------------
SEEDS = {"a": 1, "b": 2, "c": 11, "d": 4}
SHAPES = {"a": (24, 40), "b": (24, 40), "c": (21, 37), "d": (5, 7)}


def scene(name):
    """The depth cases: (depth [2,H,W], Kinv [2,3,3], proj [2,3,4], holes [2,H,W] | None, the depth before the holes | None), float32
    numpy.  A box at 5 m on a slanted 18-25 m background seen from a camera 0.54 m to the side (f = 0.75 W); b, c: plus a yaw of
    2 degrees and 0.3 m forward; c: 10 % of the source depths are 0 (holes = 1 there)."""
    H, W = SHAPES[name]
    rng = np.random.RandomState(SEEDS[name])
    B = 2
    f = 0.75 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], dtype=np.float64)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = np.zeros((B, H, W))
    for b in range(B):
        near, far = 18.0 + rng.rand(), 24.0 + rng.rand()
        slant = xs / (W - 1.0) if b == 0 else 1.0 - xs / (W - 1.0)
        depth[b] = near + (far - near) * slant + 0.3 * ys / (H - 1.0)
        h0, w0 = rng.randint(H // 6, H // 3), rng.randint(W // 5, W // 2)
        depth[b, h0:h0 + max(H // 3, 2), w0:w0 + max(W // 4, 2)] = 5.0 + 0.1 * rng.rand()
    pose = np.eye(4)
    pose[0, 3] = 0.54
    if name in ("b", "c"):
        a = np.deg2rad(2.0)
        pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        pose[2, 3] = -0.3   # the camera moves forward: the points come closer and the image expands
    holes, full = None, None
    if name == "c":
        holes = (rng.rand(B, H, W) < 0.10).astype(np.float32)
        full = depth.astype(np.float32)
        depth = depth * (1 - holes)
    Kinv = np.broadcast_to(np.linalg.inv(K), (B, 3, 3))
    proj = np.broadcast_to(K @ pose[:3], (B, 3, 4))
    return depth.astype(np.float32), np.ascontiguousarray(Kinv, dtype=np.float32), np.ascontiguousarray(proj, dtype=np.float32), holes, full


def flows(name):
    """The generic cases on 16 x 16, B = 2: the flow [2,2,16,16] (float32 numpy) whose positions are base grid + flow, exactly."""
    B, H, W = 2, 16, 16
    rng = np.random.RandomState({"e_int": 11, "e_quarter": 12, "e_collide": 13, "e_edge": 14, "e_nonfinite": 15}[name])
    base = base_grid(B, H, W).numpy()
    if name == "e_int":      # item 0: the two-disparity scene of analytic_band; item 1: random integer flows
        flow = np.zeros((B, 2, H, W), dtype=np.float32)
        flow[0, 0] = -BAND["d_bg"]
        flow[0, 0, BAND["rows"][0]:BAND["rows"][1], BAND["cols"][0]:BAND["cols"][1]] = -BAND["d_fg"]
        flow[1] = rng.randint(-3, 4, size=(2, H, W))
        return flow
    if name == "e_quarter":
        return (rng.randint(-12, 13, size=(B, 2, H, W)) / 4.0).astype(np.float32)
    if name == "e_collide":
        pos = np.zeros((B, 2, H, W), dtype=np.float32)
        pos[:, 0], pos[:, 1] = COLLIDE_AT
        return pos - base
    if name == "e_edge":     # positions on the last row / column, one outside on either side, and a few inside
        xs = np.array([-1.0, 0.0, W - 1.0, W, 3.5, W - 1.25])
        ys = np.array([-1.0, 0.0, H - 1.0, H, 7.25, H - 1.5])
        pos = np.stack((rng.choice(xs, size=(B, H, W)), rng.choice(ys, size=(B, H, W))), 1).astype(np.float32)
        return pos - base
    if name == "e_nonfinite":
        flow = (rng.randint(-12, 13, size=(B, 2, H, W)) / 4.0).astype(np.float32)
        kind = rng.randint(0, 12, size=(B, 2, H, W))
        flow[kind == 0], flow[kind == 1], flow[kind == 2] = np.nan, np.inf, -np.inf
        return flow
    raise KeyError(name)


def analytic_band():
    """visible [16,16] of item 0 of e_int, by construction: the background moves d_bg to the left, the box d_fg; nothing lands in the
    d_fg - d_bg columns the box uncovers on its right, nor in the last d_bg columns of the image."""
    vis = np.ones((16, 16), dtype=np.float32)
    vis[:, 16 - BAND["d_bg"]:] = 0
    vis[BAND["rows"][0]:BAND["rows"][1], BAND["cols"][1] - BAND["d_fg"]:BAND["cols"][1] - BAND["d_bg"]] = 0
    return vis


def flow_pair():
    """(x [2,3,16,16], flow12, flow21 [2,2,16,16]) of the flow_warp / bidirectional-check fixture."""
    rng = np.random.RandomState(21)
    x = rng.rand(2, 3, 16, 16).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij")
    flow12 = np.stack([np.stack((sx + 0.5 * np.sin(xs / 3.0 + b), sy + 0.4 * np.cos(ys / 4.0))) for b, (sx, sy) in
                       enumerate(((1.5, -0.75), (-2.25, 1.0)))]).astype(np.float32)
    flow21 = (-flow12 + 0.45 * rng.randn(2, 2, 16, 16)).astype(np.float32)
    return x, flow12, flow21


def pos64(case):
    """The reference's float64 positions of a depth case, stored as their distance from its float32 ones."""
    return torch.from_numpy(case["pos32"]).double() + torch.from_numpy(case["pos64_minus_pos32"]).double()


_CASES = None


def cases():
    """{case name: {key: array}} of tests/golden/g27_occlusion.npz (keys `<case>.<key>`), loaded once and shared."""
    global _CASES
    if _CASES is None:
        out = {}
        with np.load(GOLDEN) as z:
            for k in z.files:
                name, key = k.split(".", 1)
                out.setdefault(name, {})[key] = z[k]
        _CASES = out
    return _CASES
