"""Restatements of ops.lidar_depth for the tests (numpy + torch on the CPU): the formulas of include/pdepth.h in float64 and, in two
summation orders, in float32; the first-order fp32 error bound of a point's position; a synthetic 64-beam scan with a KITTI-like
calibration; and the case generator that removes every point whose pixel, z test or filter decision an fp32 rounding could flip.

The reference's extension (external/utils_lib, Eigen + OpenCV + pybind11) cannot be built where these tests run, so there is no
golden fixture from it: the contract is its source, restated here."""
import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = np.float32, np.float64
EPS32 = float(np.finfo(np.float32).eps)   # 2^-23
# a chain of four products and three sums, in any order, fused or not: |error| <= gamma_4 sum |terms| < 4 EPS32 sum |terms|
# (gamma_4 = 4u / (1 - 4u) with u = EPS32 / 2: the factor 4 EPS32 has a factor 2 in hand)
CHAIN = 4.0 * EPS32


def cast_inputs(points, M, intr):
    """What the binding hands the kernels: fp32 points [N,4] (w = 1 appended to [N,3]), M [4,4], intr [3,4] (zero column appended)."""
    points = np.asarray(points, dtype=F32)
    if points.shape[1] == 3:
        points = np.concatenate([points, np.ones((len(points), 1), F32)], axis=1)
    intr = np.asarray(intr, dtype=F32)
    if intr.shape[1] == 3:
        intr = np.concatenate([intr, np.zeros((3, 1), F32)], axis=1)
    return points, np.asarray(M, dtype=F32), intr


def project64(points, M, intr):
    """float64 arithmetic on the fp32 inputs -> (cam [N,4], proj [N,3], u_f, v_f)."""
    p, M, I = points.astype(F64), M.astype(F64), intr.astype(F64)
    with np.errstate(all="ignore"):
        cam = p @ M.T
        proj = cam @ I.T
        return cam, proj, proj[:, 0] / proj[:, 2], proj[:, 1] / proj[:, 2]


def _dot4_f32(c, v, fused):
    """((c0 v0 + c1 v1) + c2 v2) + c3 v3 in fp32: every product and sum rounded (fused = False), or each step one fused
    multiply-add (the exact product of two floats fits a double; the sum is rounded to double and then to float)."""
    with np.errstate(all="ignore"):
        acc = (c[0] * v[0]).astype(F32)
        for k in range(1, 4):
            if fused:
                acc = (F64(c[k]) * v[k].astype(F64) + acc.astype(F64)).astype(F32)
            else:
                acc = (acc + (c[k] * v[k]).astype(F32)).astype(F32)
    return acc


def project32(points, M, intr, fused=False):
    """The fp32 chain of include/pdepth.h (fused = False) or the same chain with fused multiply-adds -> (cam_z, u_f, v_f), fp32."""
    cols = [points[:, k] for k in range(4)]
    cam = [_dot4_f32(M[r], cols, fused) for r in range(4)]
    proj = [_dot4_f32(intr[r], cam, fused) for r in range(3)]
    with np.errstate(all="ignore"):
        return cam[2], (proj[0] / proj[2]).astype(F32), (proj[1] / proj[2]).astype(F32)


def position_bound(points, M, intr):
    """First-order bound of the fp32 error of (u_f, v_f, cam_z) per point, for either summation order.
    cam_r: CHAIN sum_k |M_rk p_k|.  proj_r: sum_k |I_rk| d cam_k + CHAIN sum_k |I_rk cam_k|.  u_f = proj_0 / proj_2:
    (d proj_0 + |u_f| d proj_2) / |proj_2| + EPS32 |u_f| for the division -- for a near point it grows as fx dX / Z."""
    cam, proj, uf, vf = project64(points, M, intr)
    Ia = np.abs(intr.astype(F64))
    with np.errstate(all="ignore"):
        dcam = CHAIN * (np.abs(points.astype(F64)) @ np.abs(M.astype(F64)).T)
        dproj = dcam @ Ia.T + CHAIN * (np.abs(cam) @ Ia.T)
        du = (dproj[:, 0] + np.abs(uf) * dproj[:, 2]) / np.abs(proj[:, 2]) + EPS32 * np.abs(uf)
        dv = (dproj[:, 1] + np.abs(vf) * dproj[:, 2]) / np.abs(proj[:, 2]) + EPS32 * np.abs(vf)
    return du, dv, dcam[:, 2]


def pixels(z, uf, vf, H, W):
    """(indices of the points that land in the image, their flat pixel): cam_z >= 0.1 and finite, u = (int)(u_f - 0.5) with the
    0.5 subtracted in double and truncation toward zero, (-1, 1) -> 0."""
    with np.errstate(all="ignore"):
        ud, vd = uf.astype(F64) - 0.5, vf.astype(F64) - 0.5
        ok = (z >= z.dtype.type(0.1)) & np.isfinite(z) & (ud > -1) & (ud < W) & (vd > -1) & (vd < H)
    idx = np.nonzero(ok)[0]
    return idx, np.trunc(vd[idx]).astype(np.int64) * W + np.trunc(ud[idx]).astype(np.int64)


def zbuffer(z, pix, H, W):
    """Per pixel the minimum z, 0 where none lands; also the index (into z) of a winner per pixel, -1 where none."""
    flat = np.full(H * W, np.inf, z.dtype)
    np.minimum.at(flat, pix, z)
    win = np.full(H * W, -1, np.int64)
    order = np.argsort(z, kind="stable")
    upix, first = np.unique(pix[order], return_index=True)
    win[upix] = order[first]
    flat[np.isinf(flat)] = 0
    return flat.reshape(H, W), win.reshape(H, W)


def window_min(zb, f):
    """Minimum of the non-empty pixels of every (2f+1)^2 window (inf where it has none), the centre included: its difference
    to itself is 0, which is never < -filterdiff for the filterdiff >= 0 these tests use."""
    t = torch.from_numpy(zb)
    lifted = torch.where(t == 0, torch.full_like(t, float("inf")), t)
    return (-F.max_pool2d(-lifted[None, None], 2 * f + 1, stride=1, padding=f))[0, 0].numpy()


def maps_from_zbuffer(zb, f, filterdiff, pool_default=1000.0):
    """Filter, masks and the quarter map of one z-buffer, in the z-buffer's dtype -> (dmap, mask, dmap_quarter, mask_quarter)."""
    assert filterdiff >= 0
    H, W = zb.shape
    dt = zb.dtype.type
    with np.errstate(all="ignore"):
        bad = (window_min(zb, f) - zb).astype(zb.dtype) < dt(-filterdiff)
    region = np.zeros((H, W), bool)
    region[f:max(H - f - 1, f), f:max(W - f - 1, f)] = True
    large = np.where(region & ~bad, zb, dt(0))
    mask = (large >= dt(0.01)).astype(zb.dtype)
    large = large * mask
    if H < 4 or W < 4:
        small = np.zeros((H // 4, W // 4), zb.dtype)
    else:
        t = torch.from_numpy(large)[None, None]
        lifted = torch.where(t == 0, torch.full_like(t, pool_default), t) if pool_default else t
        small = -F.max_pool2d(-lifted, 4)
        small = torch.where(small == pool_default, torch.zeros_like(small), small)[0, 0].numpy()
    mask_s = (small >= dt(0.01)).astype(zb.dtype)
    return large, mask, small * mask_s, mask_s


def reference(points, M, intr, H, W, f, filterdiff=1.0, pool_default=1000.0, dtype=F64, fused=False):
    """One item -> dict(dmap, mask, dmap_quarter, mask_quarter, zbuf, tol): dtype float64 = the float64 restatement (tol: per pixel
    CHAIN sum_k |M_2k p_k| of the winning point), float32 = one of the two fp32 restatements."""
    points, M, intr = cast_inputs(points, M, intr)
    if dtype is F64:
        cam, _, uf, vf = project64(points, M, intr)
        z = cam[:, 2]
    else:
        z, uf, vf = project32(points, M, intr, fused)
    idx, pix = pixels(z, uf, vf, H, W)
    zb, win = zbuffer(z[idx], pix, H, W)
    dz = position_bound(points, M, intr)[2][idx]
    tol = np.where(win >= 0, dz[np.maximum(win, 0)] if len(idx) else 0.0, 0.0)
    out = dict(zip(("dmap", "mask", "dmap_quarter", "mask_quarter"), maps_from_zbuffer(zb, f, filterdiff, pool_default)))
    out["zbuf"], out["tol"] = zb, tol
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def calibration(H, W):
    """KITTI-like: velodyne (x forward, y left, z up) -> camera (x right, y down, z forward) with a small rotation and the
    sensor offset; a pinhole with a non-zero fourth column (the rectified camera's baseline term).  float64, as a loader holds them."""
    a, b, c = 0.0075, -0.0148, 0.0012
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    M = np.eye(4)
    M[:3, :3] = Rx @ Ry @ Rz @ axes
    M[:3, 3] = [-0.004, -0.0763, -0.2718]
    fx = 0.58 * W
    intr = np.array([[fx, 0.0, 0.5 * W + 0.7, 0.0585 * fx], [0.0, 1.02 * fx, 0.5 * H + 0.3, 0.0003 * fx], [0.0, 0.0, 1.0, 0.0027]])
    return M, intr


def synthetic_scan(seed, n, half_fov_deg=180.0):
    """n points of a 64-beam scan [n,4] (w = 1), float64: beams from +2 to -24.8 degrees, azimuth within +- half_fov_deg of
    forward, over a ground plane 1.73 m below the sensor and walls of a random range per azimuth sector (depth steps: the
    occlusion filter has work)."""
    rng = np.random.default_rng(seed)
    beam = rng.integers(0, 64, n)
    elev = np.deg2rad(2.0 - 26.8 * (beam + rng.uniform(-0.05, 0.05, n)) / 63.0)
    az = np.deg2rad(rng.uniform(-half_fov_deg, half_fov_deg, n))
    sectors = rng.uniform(4.0, 60.0, 96)
    wall = sectors[((az + np.pi) / (2 * np.pi) * 96).astype(int) % 96]
    with np.errstate(divide="ignore"):
        ground = np.where(elev < 0, 1.73 / np.maximum(-np.sin(elev), 1e-9), np.inf)
    r = np.minimum(wall / np.cos(elev), ground) * (1.0 + 0.002 * rng.standard_normal(n))
    return np.stack([r * np.cos(elev) * np.cos(az), r * np.cos(elev) * np.sin(az), r * np.sin(elev), np.ones(n)], axis=1)


def prune(points, M, intr, H, W, f, filterdiff=1.0):
    """Remove every point an fp32 rounding could move across a decision: a position within twice its error bound of a pixel
    boundary (for points near the image), a cam_z within twice its bound of 0.1, and -- repeated until none is left -- the points
    of every pixel whose filter decision |zn_min - z + filterdiff| lies within twice the z bounds involved.
    Returns (kept points fp32 [n,4], dict(in_image, removed_in_image, rounds))."""
    points, M, intr = cast_inputs(points, M, intr)
    cam, _, uf, vf = project64(points, M, intr)
    du, dv, dz = position_bound(points, M, intr)
    z = cam[:, 2]
    in_image_before = len(pixels(z, uf, vf, H, W)[0])
    with np.errstate(all="ignore"):
        ud, vd = uf - 0.5, vf - 0.5
        near = (z >= 0.1 - 2 * dz) & (ud > -2) & (ud < W + 1) & (vd > -2) & (vd < H + 1)
        amb = near & ((np.abs(ud - np.rint(ud)) <= 2 * du) | (np.abs(vd - np.rint(vd)) <= 2 * dv))
        amb |= np.abs(z - 0.1) <= 2 * dz
        amb |= ~np.isfinite(z) | (near & ~(np.isfinite(ud) & np.isfinite(vd)))
    keep = ~amb
    rounds = 0
    while True:
        rounds += 1
        assert rounds <= 20
        kept = np.nonzero(keep)[0]
        idx, pix = pixels(z[kept], uf[kept], vf[kept], H, W)
        zb, win = zbuffer(z[kept][idx], pix, H, W)
        tol = np.where(win >= 0, dz[kept][idx][np.maximum(win, 0)], 0.0)
        tol_n = F.max_pool2d(torch.from_numpy(tol)[None, None], 2 * f + 1, stride=1, padding=f)[0, 0].numpy()
        with np.errstate(all="ignore"):
            margin = np.abs(window_min(zb, f) - zb + filterdiff)
        bad_pix = np.nonzero(((zb != 0) & (margin <= 2 * (tol + tol_n))).ravel())[0]
        if len(bad_pix) == 0:
            break
        keep[kept[idx[np.isin(pix, bad_pix)]]] = False
    cam_k = z[keep]
    in_image_after = len(pixels(cam_k, uf[keep], vf[keep], H, W)[0])
    return points[keep], {"in_image": in_image_before, "removed_in_image": in_image_before - in_image_after, "rounds": rounds}


def pruned_scan(seed, n, H, W, f, filterdiff=1.0, half_fov_deg=180.0):
    """-> (points fp32 [n',4], M fp32, intr fp32 [3,4], stats)."""
    M, intr = calibration(H, W)
    pts, stats = prune(synthetic_scan(seed, n, half_fov_deg), M, intr, H, W, f, filterdiff)
    _, M32, I32 = cast_inputs(pts, M, intr)
    return pts, M32, I32, stats


def back_project(M, intr, u, v, depth):
    """float64 points [n,4] (w = 1) whose float64 position is (u, v) (so u_f - 0.5 = u - 0.5) at camera depth `depth`."""
    M, I = np.asarray(M, F64), np.asarray(intr, F64)
    u, v, depth = (np.asarray(x, F64) for x in (u, v, depth))
    out = np.empty((len(u), 4))
    Minv = np.linalg.inv(M)
    for i in range(len(u)):
        # proj = I[:, :3] cam + I[:, 3] (cam_w = 1 for a rigid M); proj_0 = u proj_2, proj_1 = v proj_2, cam_z = depth
        A = np.array([I[0, :3] - u[i] * I[2, :3], I[1, :3] - v[i] * I[2, :3], [0.0, 0.0, 1.0]])
        rhs = np.array([u[i] * I[2, 3] - I[0, 3], v[i] * I[2, 3] - I[1, 3], depth[i]])
        out[i] = Minv @ np.append(np.linalg.solve(A, rhs), 1.0)
    return out
