"""Shared by tests/test_warps_host.py and tests/test_warps_gpu.py: float64 references of the two warps, the mask of the
pixels where a float32 evaluation may legitimately take another branch than float64, the yardstick (the float32 oracle's
own distance from float64) and the case tables.

warp_feature (csrc/warp.hip) is a bilinear gather at positions the suite already pins bit for bit
(test_hip_parity.py::test_sample_coordinates_bit_exact), so its reference takes the oracle's float32 positions as they are
and evaluates only the gather in float64: bilinear64.  It is written with torch ops and differentiable in `src`.

inverse_warp (csrc/inverse_warp.hip, utils/inverse_warp.py) computes its positions itself, from a depth map, so its reference is
the whole chain in float64 under autograd: inverse_warp64, the lines of oracle.ref_cpu.inverse_warp restated so that the
projected point and the sample position come back too (the host test pins the restatement to the oracle bit for bit)."""
import numpy as np
import torch
import torch.nn.functional as F

from pdepth_amd import synth
from pdepth_amd.utils import inverse_warp as iw
from oracle import ref_cpu as O

EPS32 = float(torch.finfo(torch.float32).eps)


# ---- the gather ------------------------------------------------------------------------------------------------------------
def _taps(ix, iy, H, W):
    """float32 positions -> (finite, x0, y0 clamped to [-2, size + 1] as int64, w, n: the float32 fractions as float64)."""
    ix, iy = ix.float(), iy.float()
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    x, y = torch.where(fin, ix, torch.zeros_like(ix)), torch.where(fin, iy, torch.zeros_like(iy))
    xf, yf = torch.floor(x), torch.floor(y)
    w, n = (x - xf).double(), (y - yf).double()          # (float32 subtractions: what the float32 samplers compute)
    return fin, xf.clamp(-2, W + 1).long(), yf.clamp(-2, H + 1).long(), w, n


def tap_mask(ix, iy, H, W):
    """int64, bit 0 nw, 1 ne, 2 sw, 3 se: the taps of the bilinear footprint whose integer coordinates lie inside the image
    (0 for a non-finite position).  x and y are in or out independently, so only 9 of the 15 non-empty masks exist:
    {nw, ne, sw, se alone; the two rows; the two columns; all four}."""
    fin, x0, y0, _, _ = _taps(ix, iy, H, W)
    xi0, xi1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    yi0, yi1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    m = (xi0 & yi0).long() + 2 * (xi1 & yi0).long() + 4 * (xi0 & yi1).long() + 8 * (xi1 & yi1).long()
    return torch.where(fin, m, torch.zeros_like(m))


def bilinear64(src, ix, iy, nonfinite=float("nan")):
    """Zeros-padded bilinear gather in float64.  src [L..., H, W] (any dtype, cast to float64), ix / iy [L..., S...]
    un-normalised positions -> [L..., S...] float64.  floor and the fraction come from the float32 value of the position;
    the weights (1-w)(1-n), w(1-n), (1-w)n, wn and the sum are float64.  A tap counts only if its integer coordinates lie
    inside the image; a non-finite position yields `nonfinite`.  Differentiable in src."""
    H, W = src.shape[-2:]
    lead = tuple(src.shape[:-2])
    assert tuple(ix.shape[:len(lead)]) == lead and ix.shape == iy.shape
    n_lead = int(np.prod(lead)) if lead else 1
    s = src.double().reshape(n_lead, H * W)
    fin, x0, y0, w, n = _taps(ix.reshape(n_lead, -1), iy.reshape(n_lead, -1), H, W)
    out = torch.zeros(x0.shape, dtype=torch.float64)
    for dx, dy, wt in ((0, 0, (1 - w) * (1 - n)), (1, 0, w * (1 - n)), (0, 1, (1 - w) * n), (1, 1, w * n)):
        xx, yy = x0 + dx, y0 + dy
        inside = fin & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        val = s.gather(1, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1))
        out = out + torch.where(inside, val * wt, torch.zeros_like(wt))
    out = torch.where(fin, out, torch.full_like(out, nonfinite))
    return out.reshape(ix.shape)


# ---- warp_feature ----------------------------------------------------------------------------------------------------------
def oracle_positions(batch):
    """(ix, iy) float32 [B,V,D,H,W] from oracle.ref_cpu.sample_coords, the way test_sample_coordinates_bit_exact takes them."""
    B, V, D, H, W = batch["src"].shape
    ix, iy = torch.empty(B, V, D, H, W), torch.empty(B, V, D, H, W)
    for b in range(B):
        K = batch["K"][b]
        for v in range(V):
            x, y = O.sample_coords(K, batch["R"][b, v], batch["t"][b, v], batch["rays"][b], batch["d_candi"],
                                   K.numpy()[0, 2], K.numpy()[1, 2], H, W)
            ix[b, v], iy[b, v] = x.reshape(D, H, W), y.reshape(D, H, W)
    return ix, iy


def warp_feature_exact64(batch, src=None, positions=None):
    """-> (exact [B,V,D,H,W] float64, NaN where the oracle's position is not finite; finite bool [B,V,D,H,W]): channel k of
    view v gathered at the oracle's float32 positions of plane k.  `src` replaces batch['src'] (a leaf that requires grad:
    the autograd oracle of a backward)."""
    src = batch["src"] if src is None else src
    ix, iy = oracle_positions(batch) if positions is None else positions
    return bilinear64(src, ix, iy), torch.isfinite(ix) & torch.isfinite(iy)


def warp_feature_oracle32(batch, src=None):
    """O.warp_feature, the reference's own float32 path (all D x C planes, the diagonal kept), item by item -> [B,V,D,H,W]."""
    src = batch["src"] if src is None else src
    out = []
    for b in range(src.shape[0]):
        K = batch["K"][b]
        out.append(O.warp_feature(src[b:b + 1], batch["d_candi"], batch["R"][b], batch["t"][b], K, batch["rays"][b],
                                  K.numpy()[0, 2], K.numpy()[1, 2]))
    return torch.cat(out)


def warp_feature_bound(src):
    """4 eps32 max|src[b, v]| per (b, v), broadcastable to [B,V,D,H,W]: each float32 weight (1-w, 1-n, one product) carries at
    most ~3 roundings of 2^-24, the three fmas add at most 3 more on a partial sum no larger than max|src| (the weights sum
    to 1): 6 * 2^-24 max|src| = 3 eps32 max|src|; the fourth eps32 is headroom."""
    return 4 * EPS32 * src.double().abs().amax(dim=(2, 3, 4), keepdim=True)


def launcher_nchunk(B, V, D, H, W):
    """launch_warp_feature's plane-chunk count (csrc/warp.hip), restated."""
    pixblocks = (H * W + 255) // 256
    nchunk = min(max(2048 // (pixblocks * V * B), 1), 16)
    nchunk = min(nchunk, D)
    return 1 if V * nchunk > 65535 else nchunk


def _wf(config_id, B, V, D, H, W, pose="mono", **kw):
    return synth.make_batch(config_id, B, C=D, D=D, H=H, W=W, V=V, pose=pose, **kw)


def _wf_off_centre():
    offs = ((1.3, -0.6), (-0.9, 0.4), (0.2, 1.1))
    items = [synth.make_item(56000 + i, C=16, D=16, H=33, W=47, V=2, pose="mono", cx_off=cx, cy_off=cy)
             for i, (cx, cy) in enumerate(offs)]
    out = {k: torch.stack([it[k] for it in items]) for k in ("ref", "src", "K", "R", "t", "rays", "cxcy")}
    out["d_candi"] = items[0]["d_candi"]
    return out


def _wf_extreme(kind):
    """The poses of test_hip_parity.py::test_tiled_falls_back_to_gather_on_extreme_poses ('wide' is its 'sideways')."""
    b = _wf(57, 2, 2, 16, 40, 72)
    R, t = b["R"].clone(), b["t"].clone()
    if kind == "big_rotation":
        c, s = np.cos(0.6), np.sin(0.6)
        R[:, 0] = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float32)
    elif kind == "wide":
        t[:, 0] = torch.tensor([6.0, 2.0, 0.0])
    else:
        t[:, 1] = torch.tensor([0.0, 0.0, -20.0])
    b["R"], b["t"] = R, t
    return b


# (name, maker); the maker returns a batch dict of synth.make_batch with C == D.  Sizes from the launcher's arithmetic:
# pixblocks = ceil(HW / 256), nchunk = clamp(2048 / (pixblocks V B), 1, 16), then min(nchunk, D).
WARP_FEATURE_CASES = (
    ("chunks_clamped_to_D", lambda: _wf(51, 1, 1, 5, 7, 9)),            # nchunk = D = 5, one partial block
    ("chunks16_ragged_planes", lambda: _wf(52, 1, 2, 37, 17, 23)),      # nchunk = 16, planes 16..36 on later trips, HW = 391
    ("chunks3", lambda: _wf(53, 2, 3, 8, 200, 128)),                    # pixblocks V B = 600 -> nchunk = 3
    ("one_chunk", lambda: _wf(54, 2, 3, 8, 192, 256)),                  # 1152 > 1024 -> nchunk = 1
    ("model_shape", lambda: _wf(55, 1, 2, 64, 64, 128)),                # the feedback model's own call
    ("D128", lambda: _wf(58, 1, 1, 128, 6, 20)),
    ("off_centre_items", _wf_off_centre),                               # cx_off / cy_off differ per item
    ("wide", lambda: _wf_extreme("wide")),
    ("big_rotation", lambda: _wf_extreme("big_rotation")),
    ("behind", lambda: _wf_extreme("behind")),
    ("strided_views", lambda: _wf(59, 2, 2, 9, 12, 20)),
)
WARP_FEATURE_NCHUNK = {"chunks_clamped_to_D": 5, "chunks16_ragged_planes": 16, "chunks3": 3, "one_chunk": 1}
WARP_FEATURE_EXTREME = ("wide", "big_rotation", "behind")

_CACHE = {}


def cached(key, make):
    """References are computed once and shared: treat what comes back as read-only."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def warp_feature_case(name):
    return cached(("wf", name), dict(WARP_FEATURE_CASES)[name])


def warp_feature_reference(name):
    """(exact64, finite) of a case, cached."""
    return cached(("wf64", name), lambda: warp_feature_exact64(warp_feature_case(name)))


# ---- inverse_warp ----------------------------------------------------------------------------------------------------------
def _pose_mat(pose, rot):
    return iw.pose_vec2mat(pose, rot) if pose.dim() == 2 else pose


def inverse_warp_ref(img, depth, pose, K, mode="bilinear", rot="euler", dtype=torch.float64):
    """oracle.ref_cpu.inverse_warp restated on `dtype` leaves under autograd (a [B,6] pose goes through iw.pose_vec2mat in
    `dtype`) -> dict: out, valid, the projected point X, Y, pz [B,H,W], the un-normalised position ix, iy [B,H,W], and the
    leaves img, depth, pose, K (call backward on a function of out, read their .grad)."""
    img, depth, pose, K = (t.detach().to(dtype).clone().requires_grad_(True) for t in (img, depth, pose, K))
    b, _, h, w = img.shape
    i_range = torch.arange(0, h).view(1, h, 1).expand(1, h, w).type_as(depth)
    j_range = torch.arange(0, w).view(1, 1, w).expand(1, h, w).type_as(depth)
    pix = torch.stack((j_range, i_range, torch.ones(1, h, w).type_as(depth)), dim=1)
    cam = torch.matmul(K.inverse(), pix.expand(b, 3, h, w).reshape(b, 3, -1)).reshape(b, 3, h, w)
    cam = cam * depth.unsqueeze(1)
    proj = torch.matmul(K, _pose_mat(pose, rot)[:, 0:3, :])
    pc = torch.matmul(proj[:, :, :3], cam.reshape(b, 3, -1)) + proj[:, :, -1:]
    Z = pc[:, 2].clamp(min=1e-3)
    grid = torch.stack([2 * (pc[:, 0] / Z) / (w - 1) - 1, 2 * (pc[:, 1] / Z) / (h - 1) - 1], dim=2).reshape(b, h, w, 2)
    out = F.grid_sample(img, grid, padding_mode="zeros", mode=mode, align_corners=False)
    g = grid.detach()
    return {"out": out, "valid": g.abs().max(dim=-1)[0] <= 1,
            "X": pc[:, 0].detach().reshape(b, h, w), "Y": pc[:, 1].detach().reshape(b, h, w),
            "pz": pc[:, 2].detach().reshape(b, h, w),
            "ix": ((g[..., 0] + 1) * w - 1) / 2, "iy": ((g[..., 1] + 1) * h - 1) / 2,
            "img": img, "depth": depth, "pose": pose, "K": K}


def inverse_warp64(img, depth, pose, K, mode="bilinear", rot="euler"):
    return inverse_warp_ref(img, depth, pose, K, mode, rot, torch.float64)


def stable_mask(ix, iy, pz, H, W, mode, delta=1e-3):
    """bool [B,H,W], False where a float32 evaluation may legitimately take another branch than float64:
    bilinear: ix or iy within delta of an integer (another tap set); nearest: within delta of a half-integer (another
    texel); the validity test: |xn| or |yn| within delta / W of 1; pz within 1e-6 of the 1e-3 clamp; a non-finite position.

    delta is a condition, not a measurement: ten times the ~1e-4 px the float32 position chain is estimated to be off for
    coordinates under ~100 px (about ten roundings of 2^-24 * 100, amplified by the 1 / Z division).  The host test
    (test_warps_host.py::test_float32_oracle_takes_the_float64_branches_on_stable_pixels) confirms it on every case."""
    ix, iy, pz = ix.double(), iy.double(), pz.double()
    fin = torch.isfinite(ix) & torch.isfinite(iy) & torch.isfinite(pz)
    x, y = torch.where(fin, ix, torch.zeros_like(ix)), torch.where(fin, iy, torch.zeros_like(iy))
    off = 0.5 if mode == "nearest" else 0.0
    near = lambda p: ((p - off) - torch.round(p - off)).abs() <= delta
    xn, yn = (2 * x + 1) / W - 1, (2 * y + 1) / H - 1
    edge = ((xn.abs() - 1).abs() <= delta / W) | ((yn.abs() - 1).abs() <= delta / W)
    clamp = (torch.where(fin, pz, torch.zeros_like(pz)) - 1e-3).abs() <= 1e-6
    return fin & ~near(x) & ~near(y) & ~edge & ~clamp


def _intrinsics(B, H, W):
    """[B,3,3]: focal lengths near the image size, a principal point off the centre, both different per item."""
    K = torch.zeros(B, 3, 3)
    for b in range(B):
        K[b] = torch.tensor([[0.9 * W + 0.37 * b, 0.0, W / 2.0 + 1.3 - 0.7 * b],
                             [0.0, 0.95 * H - 0.21 * b, H / 2.0 - 0.8 + 0.45 * b],
                             [0.0, 0.0, 1.0]])
    return K


def _pose44(B, t, angles=None):
    """[B,4,4] from per-item translations and (optional) per-item euler angles."""
    t = torch.tensor(t, dtype=torch.float32).reshape(B, 3)
    a = torch.zeros(B, 3) if angles is None else torch.tensor(angles, dtype=torch.float32).reshape(B, 3)
    P = torch.eye(4).repeat(B, 1, 1)
    P[:, :3] = iw.pose_vec2mat(torch.cat([t, a], dim=1), "euler")
    return P


def _iw_inputs(seed, B, C, H, W, d_lo=2.0, d_hi=30.0, positive_gout=False):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, C, H, W, generator=g)
    depth = d_lo + (d_hi - d_lo) * torch.rand(B, H, W, generator=g)
    gout = torch.randn(B, C, H, W, generator=g)
    if positive_gout:
        gout = gout.abs() + 0.5
    return {"img": img, "depth": depth, "gout": gout, "K": _intrinsics(B, H, W), "rot": "euler"}


_T3 = [(0.25, -0.15, 0.4), (-0.3, 0.2, -0.25), (0.1, 0.3, 0.6)]
_A3 = [(0.02, -0.015, 0.03), (-0.025, 0.02, -0.01), (0.01, 0.03, 0.02)]


def _iw_smallest():
    """2 x 2, the smallest size the C ABI accepts.  ix = 2 u - 0.5 there, so a tap set inside the image needs u in
    (0.25, 0.75): the camera steps back 15 m from a 9..11 m scene, which shrinks the image to ~0.4 of its size around the
    principal point."""
    c = _iw_inputs(6101, 1, 1, 2, 2, 9.0, 11.0)
    c["K"] = torch.tensor([[[2.0, 0.0, 0.54], [0.0, 2.0, 0.47], [0.0, 0.0, 1.0]]])
    c["pose"] = _pose44(1, [(0.05, -0.04, 15.0)])
    return c


def _iw_ragged():
    c = _iw_inputs(6102, 3, 5, 19, 27)
    c["pose"] = _pose44(3, _T3, _A3)
    return c


def _iw_rot(rot):
    c = _iw_inputs(6103, 2, 3, 20, 28)
    c["pose"] = torch.tensor([[0.3, -0.2, 0.5, 0.10, -0.08, 0.12], [-0.25, 0.15, -0.3, -0.09, 0.11, -0.10]])
    c["rot"] = rot
    return c


def _iw_zoom():
    """The camera steps back 30 m from a ~10 m scene: the 24 x 40 target lands on a 6 x 10 patch of the source, every tap
    inside the image, 16 pixels (64 atomics) per texel.  The upstream gradient is positive so that the sum of g_img over
    the image (= the sum of gout, the weights of a sample sum to 1) is a scale to measure lost atomics against."""
    c = _iw_inputs(6104, 1, 2, 24, 40, 9.9, 10.1, positive_gout=True)
    c["pose"] = _pose44(1, [(0.37, -0.23, 30.0)])
    return c


def _iw_border():
    """Item 0: a step of 0.29 m towards a ~10 m scene magnifies by 1.03, so the outermost ring of pixels samples the 1 px
    strip around the image: every edge and corner.  Item 1: a step back of 110 m shrinks the target to a 2 x 1.3 px patch
    laid over the top right corner.  Together about half the pixels have some but not all taps inside."""
    c = _iw_inputs(6105, 2, 3, 16, 24, 9.95, 10.05)
    K = c["K"]
    # item 1: u = cx + (x - cx) / 12 + fx tx / 120 must span ix = 1.0435 u - 0.5 in (22.3, 23.9): u in (21.85, 23.4);
    # v = cy + (y - cy) / 12 + fy ty / 120 must span iy = 1.0667 v - 0.5 in (-0.9, 0.45): v in (-0.37, 0.89)
    cx, cy, fx, fy = float(K[1, 0, 2]), float(K[1, 1, 2]), float(K[1, 0, 0]), float(K[1, 1, 1])
    tx = (22.62 - (cx + (11.5 - cx) / 12.0)) * 120.0 / fx
    ty = (0.26 - (cy + (7.5 - cy) / 12.0)) * 120.0 / fy
    c["pose"] = _pose44(2, [(0.0, 0.0, -0.29), (tx, ty, 110.0)])
    return c


def _iw_outside_far():
    c = _iw_inputs(6126, 1, 2, 9, 11)
    c["pose"] = _pose44(1, [(1.0e6, 0.3, 0.0)])
    return c


def _iw_behind():
    """The camera steps 4 m forward.  45 % of the pixels (seeded) are 1..3 m away and end up behind it (pz < 1e-3); the
    others are 60..100 m away and stay where they were, to within a pixel."""
    c = _iw_inputs(6107, 1, 2, 12, 18)
    g = torch.Generator().manual_seed(6117)
    near = torch.rand(1, 12, 18, generator=g) < 0.45
    u = torch.rand(1, 12, 18, generator=g)
    c["depth"] = torch.where(near, 1.0 + 2.0 * u, 60.0 + 40.0 * u)
    c["pose"] = _pose44(1, [(0.3, -0.2, -4.0)], [(0.01, -0.02, 0.015)])
    return c


NAN_DEPTH_PIXELS = ((0, 3, 5, float("nan")), (0, 6, 9, float("inf")), (0, 8, 12, float("-inf")))


def _iw_nan_depth():
    """One NaN and one inf depth pixel in item 0 (and one -inf: behind the clamp Z = 1e-3 it is the one that makes the
    POSITION infinite rather than NaN)."""
    c = _iw_inputs(6108, 2, 3, 10, 14)
    # item 0's angles keep every entry of K @ R positive: right of and below the principal point the -inf depth then gives
    # X = Y = pz = -inf (no inf - inf), Z = 1e-3 and a position of -inf
    c["pose"] = _pose44(2, _T3[:2], [(0.02, -0.015, 0.005), _A3[1]])
    c["depth_finite"] = c["depth"].clone()
    for (b, y, x, val) in NAN_DEPTH_PIXELS:
        c["depth"][b, y, x] = val
    return c


# (name, maker); the maker returns dict(img [B,C,H,W], depth [B,H,W], pose [B,4,4] | [B,6], K [B,3,3], rot, gout)
INVERSE_WARP_CASES = (
    ("smallest", _iw_smallest),
    ("ragged", _iw_ragged),                      # HW = 513: three blocks, the last holds one pixel
    ("rot_euler", lambda: _iw_rot("euler")),
    ("rot_quat", lambda: _iw_rot("quat")),
    ("zoom_many_to_one", _iw_zoom),
    ("border", _iw_border),
    ("outside_far", _iw_outside_far),
    ("behind", _iw_behind),
    ("nan_depth", _iw_nan_depth),
)
MODES = ("bilinear", "nearest")
QUANTITIES = ("out", "g_img", "g_depth", "g_pose", "g_K")


def inverse_warp_case(name):
    return cached(("iw", name), dict(INVERSE_WARP_CASES)[name])


def _grads(r, gup):
    """Run the backward of a reference dict with upstream gradient gup -> the five quantities (detached)."""
    (r["out"] * gup.to(r["out"].dtype)).sum().backward()
    z = lambda leaf: torch.zeros_like(leaf) if leaf.grad is None else leaf.grad
    return {"out": r["out"].detach(), "g_img": z(r["img"]), "g_depth": z(r["depth"]), "g_pose": z(r["pose"]), "g_K": z(r["K"])}


def inverse_warp_reference(name, mode):
    """Cached float64 evaluation of a case: dict(M stable mask, gup = gout * M, q = the five quantities in float64, valid,
    ix, iy, pz, X, Y, taps)."""
    def make():
        c = inverse_warp_case(name)
        r = inverse_warp64(c["img"], c["depth"], c["pose"], c["K"], mode, c["rot"])
        H, W = c["img"].shape[-2:]
        M = stable_mask(r["ix"], r["iy"], r["pz"], H, W, mode)
        gup = c["gout"] * M.unsqueeze(1)
        return {"M": M, "gup": gup, "q": _grads(r, gup), "valid": r["valid"], "ix": r["ix"], "iy": r["iy"], "pz": r["pz"],
                "X": r["X"], "Y": r["Y"], "taps": tap_mask(r["ix"], r["iy"], H, W)}
    return cached(("iw64", name, mode), make)


def element_mask(quantity, M, like):
    """Where a quantity is compared: per element on M for out, g_depth; everywhere for g_img (the upstream gradient is zero
    outside M, so nothing unstable is scattered) and for the sums g_pose, g_K."""
    if quantity == "out":
        return M.unsqueeze(1).expand_as(like)
    if quantity == "g_depth":
        return M
    return torch.ones_like(like, dtype=torch.bool)


def masked_err(got, want, mask):
    """max |got - want| over mask & isfinite(want) (0.0 for an empty selection); got cast to float64."""
    sel = mask & torch.isfinite(want)
    if not bool(sel.any()):
        return 0.0
    return float((got.double() - want)[sel].abs().max())


def masked_scale(want, mask):
    sel = mask & torch.isfinite(want)
    return float(want[sel].abs().max()) if bool(sel.any()) else 0.0


def oracle32_yardstick(name, mode):
    """The float32 oracle (O.inverse_warp in float32 under autograd, the pose vector through iw.pose_vec2mat) against
    inverse_warp64, upstream gradient zero outside the stable mask -> dict(e_ref {quantity: max |f32 - f64|}, scale
    {quantity: max |f64|}, valid32, out32).  Cached; the GPU test takes its bounds from here."""
    def make():
        c = inverse_warp_case(name)
        ref = inverse_warp_reference(name, mode)
        img, depth, pose, K = (c[k].detach().clone().requires_grad_(True) for k in ("img", "depth", "pose", "K"))
        out, valid = O.inverse_warp(img, depth, _pose_mat(pose, c["rot"]), K, mode)
        q32 = _grads({"out": out, "img": img, "depth": depth, "pose": pose, "K": K}, ref["gup"])
        e_ref, scale = {}, {}
        for k in QUANTITIES:
            m = element_mask(k, ref["M"], ref["q"][k])
            e_ref[k], scale[k] = masked_err(q32[k], ref["q"][k], m), masked_scale(ref["q"][k], m)
        return {"e_ref": e_ref, "scale": scale, "valid32": valid, "q32": q32}
    return cached(("iw32", name, mode), make)


def inverse_warp_bound(name, mode, quantity):
    """max(f e_ref, 4 eps32 scale) with f = 4 for the per-element quantities and f = 16 for the sums g_pose and g_K: see
    tests/test_warps_gpu.py."""
    y = oracle32_yardstick(name, mode)
    f = 16 if quantity in ("g_pose", "g_K") else 4
    return max(f * y["e_ref"][quantity], 4 * EPS32 * y["scale"][quantity])
