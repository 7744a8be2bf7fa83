"""flow_warp, the forward-backward check, the first-order smoothness and the unsupervised flow loss restated from their
definitions in plain torch, for tests/test_flow_host.py, tests/test_flow_gpu.py, the fixture maker
(tests/golden/make_golden_flow.py) and the baselines of tools/bench_flow.py.

  flow_warp_ref      x sampled at base grid + flow, in the dtype of the flow: float64 = the tests' reference.  Written from the
                     definition (include/pdepth.h): position, clamp, floor, four weights, four masked gathers; differentiable in x and
                     in the flow by autograd (torch.clamp passes the gradient at the boundary itself, the header's rule)
  positions          the un-normalised, unclamped sample positions (ix, iy)
  fb_check_ref       (occ, margin |lhs - rhs|) of the forward-backward check
  smooth_ref         smooth_grad_1st
  unflow_ref         the loss of losses/flow_loss.py over flow_warp_ref, util_occlusion.range_map, util_ssim.ssim_dist,
                     util_ternary.ternary_dist and smooth_ref: (total, warp, smooth, mean |flow|), and the least margins of its masks
  warp_inputs        the seeded inputs of a warp case: x, flow with the planted positions, grad_out, the mask of planted pixels
  fb_inputs, smooth_inputs, unflow_inputs, train_images
  cases              tests/golden/g28_flow.npz by case name
"""
import itertools
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import util_occlusion as UO
import util_ssim as US
import util_ternary as UT

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g28_flow.npz")
EPS32 = float(torch.finfo(torch.float32).eps)
PADS = ("border", "zeros")
# (B, C, H, W): the minimum; odd sizes, W no multiple of 4; more than one wave per row and more than one block; the channel split
# (the second is the flow network's coarsest level)
SHAPES = ((3, 1, 2, 2), (2, 3, 19, 27), (1, 5, 33, 70), (1, 67, 8, 12), (2, 192, 4, 8))
FB_SHAPES = ((2, 19, 27), (2, 33, 70), (3, 16, 16))
SMOOTH_SHAPE = (2, 2, 19, 27)
NEAR = 1e-4          # grad_flow is not compared where the float64 position is this close to an integer or a clamp boundary
STORE_CAP = 256      # the fixture keeps at most this many elements of a reference output (subset: every k-th element)


def shape_key(shape):
    return "x".join(str(int(s)) for s in shape)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def positions(flow):
    """flow [B,2,H,W] -> (ix, iy) [B,H,W], un-normalised and unclamped: g = 2 v / (W - 1) - 1, ix = ((g + 1) W - 1) / 2."""
    B, _, H, W = flow.shape
    v = UO.base_grid(B, H, W, dtype=flow.dtype, device=flow.device) + flow
    gx, gy = 2 * v[:, 0] / (W - 1) - 1, 2 * v[:, 1] / (H - 1) - 1
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2


def flow_warp_ref(x, flow, pad="border"):
    B, C, H, W = x.shape
    ix, iy = positions(flow)
    finite = torch.isfinite(ix) & torch.isfinite(iy)
    ix, iy = torch.where(finite, ix, torch.full_like(ix, -8.0)), torch.where(finite, iy, torch.full_like(iy, -8.0))
    if pad == "border":
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    else:
        assert pad == "zeros"
    x0, y0 = torch.floor(ix).detach(), torch.floor(iy).detach()
    w, e, n, s = ix - x0, (x0 + 1) - ix, iy - y0, (y0 + 1) - iy
    planes = x.reshape(B, C, H * W)
    out = 0
    for tx, ty, wt in ((x0, y0, e * s), (x0 + 1, y0, w * s), (x0, y0 + 1, e * n), (x0 + 1, y0 + 1, w * n)):
        inside = finite & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
        at = (ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)).long().view(B, 1, H * W).expand(B, C, H * W)
        out = out + planes.gather(2, at) * (wt * inside.to(wt.dtype)).view(B, 1, H * W)
    return out.view(B, C, H, W)


def near_jump(flow64, pad):
    """[B,H,W] bool: the float64 position lies within NEAR of an integer (either coordinate) or, border padding, of a clamp boundary
    -- where d out / d flow jumps."""
    _, _, H, W = flow64.shape
    ix, iy = positions(flow64.double())
    bad = ~(torch.isfinite(ix) & torch.isfinite(iy))
    for p, size in ((ix, W), (iy, H)):
        # where the coordinate matters: up to the clamp boundaries (border: beyond them the position is the boundary itself, on
        # both sides of the comparison), up to the last position with a tap inside (zeros)
        live = (p > -NEAR) & (p < size - 1 + NEAR) if pad == "border" else (p > -1 - NEAR) & (p < size + NEAR)
        bad = bad | (live & ((p - p.round()).abs() < NEAR))
    return bad


def fb_check_ref(flow12, flow21, scale=0.01, bias=0.5):
    w = flow_warp_ref(flow21, flow12, "zeros")
    lhs = ((flow12 + w) ** 2).sum(1, keepdim=True)
    rhs = scale * ((flow12 ** 2).sum(1, keepdim=True) + (w ** 2).sum(1, keepdim=True)) + bias
    return (lhs > rhs).float(), (lhs - rhs).abs()


def smooth_ref(flo, image, alpha):
    wx = torch.exp(-alpha * (image[..., 1:] - image[..., :-1]).abs().mean(1, keepdim=True))
    wy = torch.exp(-alpha * (image[..., 1:, :] - image[..., :-1, :]).abs().mean(1, keepdim=True))
    dx, dy = flo[..., 1:] - flo[..., :-1], flo[..., 1:, :] - flo[..., :-1, :]
    return (wx * dx.abs()).mean() / 4 + (wy * dy.abs()).mean() / 4


def unflow_ref(cfg, flows, target):
    """-> ((total, warp, smooth, mean |flow|), least margin of the first scale's masks): threshold margin of the range map
    (occ_from_back) or |lhs - rhs| of the check."""
    images = (target[:, :3], target[:, 3:])
    first, margin, warp_terms, smooth_terms, s = None, float("inf"), [], [], 1.0

    def photo(im, recons, m):
        total = 0
        if cfg.w_l1 > 0:
            total = total + (cfg.w_l1 * (im - recons).abs() * m).mean()
        if cfg.w_ssim > 0:
            total = total + (cfg.w_ssim * US.ssim_dist(recons * m, im * m, 1)).mean()
        if cfg.w_ternary > 0:
            total = total + (cfg.w_ternary * UT.ternary_dist(recons * m, im * m, 1)).mean()
        # (a mask is float32 in the reference and in the package whatever the images are: its mean, count / n, is rounded to float32)
        return total / m.float().mean()

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
                    margin = min(margin, float((r - 0.2).abs().min()))
                else:
                    occ, m = fb_check_ref(a, b)
                    masks.append(1 - occ.to(flow.dtype))
                    margin = min(margin, float(m.min()))
            first, s = masks, min(h, w)
        else:
            masks = [F.interpolate(m, (h, w), mode="nearest") for m in first]
        warp = photo(im1, flow_warp_ref(im2, fwd, cfg.warp_pad), masks[0])
        smooth = smooth_ref(fwd / s, im1, cfg.alpha)
        if cfg.with_bk:
            warp = (warp + photo(im2, flow_warp_ref(im1, bwd, cfg.warp_pad), masks[1])) / 2
            smooth = (smooth + smooth_ref(bwd / s, im2, cfg.alpha)) / 2
        warp_terms.append(warp * cfg.w_scales[i])
        smooth_terms.append(smooth * cfg.w_sm_scales[i])
    warp_loss, smooth_loss = sum(warp_terms), cfg.w_smooth * sum(smooth_terms)
    return (warp_loss + smooth_loss, warp_loss, smooth_loss, flows[0].abs().mean()), margin


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def chain(base, f, size):
    """The position of the kernels' chain (include/pdepth.h): formed in double from the fp32 flow, v size / (size - 1) - 0.5."""
    v = np.asarray(base, np.float64) + np.asarray(f, np.float32).astype(np.float64)
    return v * (np.float64(size) / np.float64(size - 1)) - 0.5


def _aim(base, size, target, side):
    """The fp32 flow that puts pixel `base` of an axis of `size` at position `target` of the kernels' chain: as exactly as an fp32
    flow can (side 0: the closest there is), or on the nearest reachable position below (-1) / above (+1)."""
    f0 = np.float32((target + 0.5) * (size - 1) / size - base)
    steps = [f0]
    lo = hi = f0
    for _ in range(8):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        steps += [lo, hi]
    cand = np.unique(np.array(steps, np.float32))
    pos = chain(base, cand, size)
    t = float(target)
    if side == 0:
        return cand[np.argmin(np.abs(pos - t))]
    ok = pos < t if side < 0 else pos > t
    if not ok.any():
        return cand[0 if side < 0 else -1]
    return cand[ok][np.argmax(pos[ok])] if side < 0 else cand[ok][np.argmin(pos[ok])]


def _plants(H, W):
    """What is planted, most important first: per plant the (kind, argument) of the x and of the y coordinate; None keeps the
    random flow.  Kinds: ('at', t, side) a position of the chain, ('flow', value)."""
    X, Y = W - 1, H - 1
    out = [(("at", "int", 0), ("at", "int", 0)), (("at", 0, 0), None), (("at", X, 0), None), (None, ("at", 0, 0)), (None, ("at", Y, 0))]
    for t, side in itertools.product((0, None), (-1, 1)):
        out.append((("at", X if t is None else t, side), None))
        out.append((None, ("at", Y if t is None else t, side)))
    out += [(("at", -1.7, 0), None), (("at", W + 0.6, 0), None), (None, ("at", -1.3, 0)), (None, ("at", H + 0.8, 0)),
            (("flow", 1e6), None), (None, ("flow", -1e6)), (("at", "int", 0), None), (None, ("at", "int", 0)),
            (("at", 0, 0), ("at", Y, 0)), (("at", X, 0), ("at", 0, 0))]
    return out


def warp_inputs(shape):
    """x, flow, grad_out (float32 numpy) and planted [B,H,W] bool of a warp case.  Flows are N(0, 3 px); planted on top, at pixels
    spread over the batch (at most every second pixel): exact integer positions, positions exactly at 0 and at W - 1 / H - 1 and one
    representable position either side, positions leaving the image on each side, a flow of +-1e6."""
    B, C, H, W = shape
    rs = np.random.RandomState(2800 + SHAPES.index(tuple(shape)))
    x = rs.randn(B, C, H, W).astype(np.float32)
    flow = (3.0 * rs.randn(B, 2, H, W)).astype(np.float32)
    go = rs.randn(B, C, H, W).astype(np.float32)
    plants = _plants(H, W)
    n = min(len(plants), (B * H * W) // 2)
    planted = np.zeros((B, H, W), bool)
    for k, at in enumerate(np.linspace(0, B * H * W - 1, n).astype(int)):
        b, rem = divmod(int(at), H * W)
        y, xx = divmod(rem, W)
        planted[b, y, xx] = True
        for axis, (what, base, size) in enumerate(((plants[k][0], xx, W), (plants[k][1], y, H))):
            if what is None:
                continue
            if what[0] == "flow":
                flow[b, axis, y, xx] = what[1]
            else:
                t = (base + 3 + k) % size if what[1] == "int" else what[1]
                flow[b, axis, y, xx] = _aim(base, size, t, what[2])
    return x, flow, go, planted


def _upsampled_noise(rs, B, C, H, W, gh=4, gw=5):
    coarse = torch.from_numpy(rs.randn(B, C, gh, gw).astype(np.float32))
    return F.interpolate(coarse, (H, W), mode="bilinear", align_corners=True)


def fb_inputs(shape):
    """flow12: a bilinear upsampling of 3 N(0, 1) on a 4 x 5 grid; flow21 = -flow12 + 0.6 N(0, 1).  float32 numpy."""
    B, H, W = shape
    rs = np.random.RandomState(2850 + FB_SHAPES.index(tuple(shape)))
    f12 = 3.0 * _upsampled_noise(rs, B, 2, H, W)
    f21 = -f12 + 0.6 * torch.from_numpy(rs.randn(B, 2, H, W).astype(np.float32))
    return f12.numpy(), f21.numpy()


def smooth_inputs():
    B, Cf, H, W = SMOOTH_SHAPE
    rs = np.random.RandomState(2870)
    flo = rs.randn(B, Cf, H, W).astype(np.float32)
    flo[0, 0, 3, 4:9] = flo[0, 0, 3, 4]   # equal neighbours: sign(0) = 0
    flo[1, 1, 5:9, 7] = flo[1, 1, 5, 7]
    image = (0.5 + 0.25 * _upsampled_noise(rs, B, 3, H, W).numpy() + 0.02 * rs.randn(B, 3, H, W)).astype(np.float32)
    return flo, image, 10.0


def smooth_image(B, H, W, seed):
    """[B,3,H,W] in (0, 1): low-frequency noise, bicubically smooth enough for a photometric loss to have a slope."""
    rs = np.random.RandomState(seed)
    return torch.sigmoid(1.5 * _upsampled_noise(rs, B, 3, H, W, 5, 7)).numpy().astype(np.float32)


UNFLOW_SHAPES = ((24, 40), (12, 20), (6, 10))
UNFLOW_SEED = 2925   # (the maker asserts the margins of the masks and of the positions for this seed; one that breaks them is changed)
UNFLOW_CASES = tuple(itertools.product((True, False), (True, False), PADS))   # (occ_from_back, with_bk, warp_pad)


def unflow_cfg(occ_from_back, with_bk, warp_pad):
    return types.SimpleNamespace(w_l1=0.15, w_ssim=0.85, w_ternary=0.5, alpha=10, warp_pad=warp_pad, occ_from_back=occ_from_back,
                                 with_bk=with_bk, w_scales=[1, 1, 0.5], w_sm_scales=[1, 0, 0], w_smooth=10)


def unflow_name(occ_from_back, with_bk, warp_pad):
    return "unflow_%s_%s_%s" % ("back" if occ_from_back else "fb", "bk" if with_bk else "fwd", warp_pad)


def unflow_inputs(seed=UNFLOW_SEED):
    """(flows: three levels [2,4,h,w], target [2,6,24,40]), float32 numpy: a smooth image pair and smooth flows of a few pixels
    (less at the coarser levels), the backward flow roughly the negative of the forward one."""
    B = 2
    rs = np.random.RandomState(seed)
    H, W = UNFLOW_SHAPES[0]
    target = np.concatenate((smooth_image(B, H, W, seed + 1), smooth_image(B, H, W, seed + 2)), 1)
    flows = []
    for i, (h, w) in enumerate(UNFLOW_SHAPES):
        fwd = (2.5 / 2 ** i) * _upsampled_noise(rs, B, 2, h, w)
        bwd = -fwd + (0.5 / 2 ** i) * _upsampled_noise(rs, B, 2, h, w)
        flows.append(torch.cat((fwd, bwd), 1).numpy().astype(np.float32))
    return flows, target


def train_images(B=2, H=24, W=40, shift=(2, 1)):
    """target [B,6,H,W]: a smooth image and its copy shifted by (dx, dy) = shift pixels (cut from one wider image)."""
    dx, dy = shift
    wide = smooth_image(B, H + dy, W + dx, 2890)
    return np.concatenate((wide[:, :, dy:, dx:], wide[:, :, :H, :W]), 1).copy()


def subset(a, cap=STORE_CAP):
    """Every k-th element of the flattened array, at most `cap` of them (all of a small array)."""
    flat = np.asarray(a).reshape(-1)
    return flat[::max(1, -(-flat.size // cap))]


def tol(ref_err, scale, floor_eps=8):
    """The tests' tolerance: twice the reference's own fp32 error, with a floor of floor_eps eps32 scale."""
    return max(2.0 * float(ref_err), floor_eps * EPS32 * float(scale))


def ref64(case, key):
    """The reference's float64 result of a fixture entry (stored as its float32 result plus a float32 difference), as a tensor."""
    v32, d = case[key + "32"], case[key + "64d"]
    if v32.size != d.size:   # (a float32 result kept whole: the difference covers its subset)
        v32 = subset(v32)
    return torch.from_numpy(v32).double() + torch.from_numpy(d).double()


_CASES = None


def cases():
    """{case name: {key: array}} of tests/golden/g28_flow.npz (keys `<case>.<key>`), loaded once and shared."""
    global _CASES
    if _CASES is None:
        out = {}
        with np.load(GOLDEN) as z:
            for k in z.files:
                name, key = k.split(".", 1)
                out.setdefault(name, {})[key] = z[k]
        _CASES = out
    return _CASES
