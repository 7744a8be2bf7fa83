"""Shared by the suites of the sweep backward (csrc/sweep_bwd.hip): autograd of the oracle's formula in float64 / fp32, the
HIP gradients, the error measure and its L1 allowance; and a host restatement of how the g_src pass of the kernel groups the
planes of a (tile, view) pair -- staged through the LDS box image, added directly, or empty -- with the inputs that reach the
paths the ordinary poses never take (tests/test_sweep_backward_groups.py).

The per-element criterion (tests/test_sweep_backward_host.py, tests/test_sweep_backward_pin_gpu.py).  The reference is
exact64_grads: float64 arithmetic at the float32 sample positions of oracle.ref_cpu.sample_coords, which the kernel, the
reference's float32 grid_sample and this module all have bit for bit -- so no tolerance pays for positions an ulp apart, as
the float64 grid_sample of oracle_cost makes it do.  Per sample (item, view, plane, pixel, channel): g the upstream gradient,
c = (2 | 1) / |sigma|, w_t the in-bounds taps' weights, s_t their texels, r the reference feature, S = sum_t w_t |s_t|,
e = sum_t w_t s_t - r.  The contributions are q_t = g c w_t e to g_src at tap t and -g c e to g_ref (L1: sign(e) for e).
With u = 2^-24, counted on csrc/sweep_bwd_body.hpp and geometry.hpp::make_footprint, first order in u:
  weights  w = ix - floor(ix) is exact (floor(ix) <= ix < floor(ix) + 1, both on ix's grid or a finer one); 1 - w is one
           rounding; a weight is the product of two such factors: one rounding more, so a weight carries at most 3 u;
  value    val = vnw nw, then three fmas: 4 roundings on partial sums bounded by S, so |d val| <= 3 u S + 4 u S = 7 u S;
           e = val - r is one more rounding: |d e| <= 7 u S + u |e|;
  factors  gscale = (2 | 1) / sigma, coef = g gscale, r = coef e, q = w r: 4 roundings, the weight's 3 u and the u |e| of the
           subtraction: 8 u relative to the contribution (g_ref: 5 u; L1, where r = +-coef: 6 u and 2 u) -- 8 u bounds all;
  sum      n terms added in any order in float32: at most n u sum |q|.  (The kernel does better: g_ref sums a view's planes in
           double, the float path's box image is double and is rounded once per flush, the integer sum is exact with at most two
           roundings of the conversion; float32 adds remain between views, groups and tiles, and in torch's own sum.)
Summed over the samples that reach an element, A0 = sum |g| c w_t |e| (L1: |e| -> 1), A1 = sum |g| c w_t S (L2 only; for g_ref
w_t = 1 and n = V D), the worst case is u (7 A1 + (8 + n) A0).  The bound is twice that, eps32 (7 A1 + (8 + n) A0), which also
covers the second-order terms; it is exactly 0 where nothing contributes, and there the gradient must be exactly 0.  No constant
is fitted.  The integer sum adds its documented quantisation, n N M_b 2^-59 (fixed_accum.hpp, sweep_bwd_det.hip: N = D H W,
M_b = |gscale| max|g_cost[b]| (max|src[b]| + max|ref[b]|), L1: |gscale| max|g_cost[b]|).
L1: sign(e) is decided by val, which is off by at most 7 u S (the subtraction val - r never changes a sign).  A sample with
S > 0 and |e64| <= 7 eps32 S -- twice that -- is ambiguous: it may move g_ref by 2 |g| / |sigma| and g_src by 2 |g| w_t / |sigma| at
its taps, and the bound adds exactly that.  At most 1 % of the elements of a case may carry such an allowance."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from pdepth_amd import ops, synth
from oracle import ref_cpu as O
import util_warps as UW

EPS32 = UW.EPS32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(REPO, "probabilistic-depth_amd", "csrc", "sweep_bwd_body.hpp")   # the one body of both g_src paths


def to_dev(b, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def oracle_cost(ref, src, b, sigma, metric, dtype):
    """est_swp_volume_v4 restated on device tensors of `dtype` (grid from oracle.ref_cpu.plane_coords, fp32, cast) -> [B,D,H,W]."""
    B, V, C, H, W = src.shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    D = d32.numel()
    out = []
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        cost = 0
        for v in range(V):
            grid = O.plane_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), d32, cx, cy).reshape(D, H, W, 2)
            grid = grid.to(device=src.device, dtype=dtype)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                                   align_corners=False)
            diff = warped - ref[i].unsqueeze(0)
            dist = (diff ** 2).sum(1) if metric == "L2" else diff.abs().sum(1)
            cost = cost + dist / sigma
        out.append(cost)
    return torch.stack(out)


def oracle_grads(b, gup, sigma, metric, dtype, dev):
    ref = b["ref"].to(dev, dtype).detach().clone().requires_grad_(True)
    src = b["src"].to(dev, dtype).detach().clone().requires_grad_(True)
    (oracle_cost(ref, src, b, sigma, metric, dtype) * gup.to(dtype)).sum().backward()
    return ref.grad, src.grad


def hip_grads(d, gup, sigma, metric, algo="auto", want_ref=True, want_src=True):
    """(g_ref, g_src, cost) of ops.sweep_cost; an output that is not wanted (its input does not require grad) is None."""
    ref = d["ref"].clone().requires_grad_(want_ref)
    src = d["src"].clone().requires_grad_(want_src)
    cost = ops.sweep_cost(ref, src, d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], sigma, feat_dist=metric, algo=algo)
    (cost * gup).sum().backward()
    return ref.grad, src.grad, cost


def rel_err(g, g64, allow=None, den=None):
    """max |g - g64| / max |g64|; with `allow`, the excess over the per-element allowance (see l1_allowance); with `den`, that
    denominator instead (a part of a tensor measured against the maximum of the whole)."""
    d = (g.double() - g64).abs()
    if allow is not None:
        d = (d - allow).clamp_min(0)
    return float(d.max() / (g64.abs().max() if den is None else den))


def l1_allowance(b, gup, sigma, dev, tau=1e-5):
    """(allow_ref, allow_src): how far a correct fp32 evaluation of the L1 gradient may be from the float64 one.

    d|e|/de = sign(e) jumps at e = 0.  Where the float64 difference e of a (view, plane, pixel, channel) sample is within
    fp32 rounding of zero (|e| <= tau (1 + |ref|): some ten times the fp32 error of e), an fp32 evaluation may take the other
    branch -- sign +-1 or 0 instead of the float64 one --, a change of up to 2 g / sigma in g_ref and 2 g w_t / sigma in g_src
    at the sample's taps (about one sample in 1e5 at the shapes below).  The allowance is exactly that bound, summed over the
    ambiguous samples; every other element is held to the plain criterion."""
    dt = torch.float64
    ref = b["ref"].to(dev, dt)
    src = b["src"].to(dev, dt).detach().clone().requires_grad_(True)
    B, V, C, H, W = src.shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    D = d32.numel()
    g = gup.to(dev, dt).abs() * (2.0 / sigma)
    allow_ref = torch.zeros_like(ref)
    total = 0
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            grid = O.plane_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), d32, cx, cy).reshape(D, H, W, 2)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid.to(dev, dt), mode="bilinear",
                                   padding_mode="zeros", align_corners=False)
            amb = ((warped.detach() - ref[i].unsqueeze(0)).abs() <= tau * (1 + ref[i].abs().unsqueeze(0))).to(dt)
            w = amb * g[i].unsqueeze(1)                                     # [D,C,H,W]
            allow_ref[i] += w.sum(0)
            total = total + (w * warped).sum()                              # d/dsrc = the taps' weights times w
    total.backward()
    return allow_ref, src.grad


# ---- float64 at the kernel's positions, and the bound an fp32 evaluation is held to, element by element ----------------------
def case_positions(b):
    """(ix, iy) float32 [B,V,D,H*W] of oracle.ref_cpu.sample_coords: the positions every fp32 implementation has bit for bit."""
    B, V, C, H, W = b["src"].shape
    ix, iy = [], []
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            x, y = O.sample_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), b["d_candi"], cx, cy, H, W)
            ix.append(x)
            iy.append(y)
    D = ix[0].shape[0]
    return torch.stack(ix).reshape(B, V, D, H * W), torch.stack(iy).reshape(B, V, D, H * W)


def oracle_positions64(b):
    """(ix, iy) float64 [B,V,D,H*W]: where a float64 grid_sample puts the samples of oracle_cost -- the float32 grid of
    oracle.ref_cpu.plane_coords un-normalised in float64, ((g + 1) size - 1) / 2."""
    B, V, C, H, W = b["src"].shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    ix, iy = [], []
    for i in range(B):
        K = b["K"][i].cpu()
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            g = O.plane_coords(K, b["R"][i, v].cpu(), b["t"][i, v].cpu(), b["rays"][i].cpu(), d32, cx, cy).double()
            ix.append(((g[..., 0] + 1) * W - 1) / 2)
            iy.append(((g[..., 1] + 1) * H - 1) / 2)
    return torch.stack(ix).reshape(B, V, -1, H * W), torch.stack(iy).reshape(B, V, -1, H * W)


def _tap_list(ix, iy, H, W):
    """Positions [d,HW] (float32: floor and fraction are taken in float32, where the subtraction is exact; float64: taken as they
    are) -> the four taps as (inside bool, flat texel index int64, weight float64), each [d,HW].  A tap outside the image or of
    a position that is not finite is not inside; the weights (1-w)(1-n), w(1-n), (1-w)n, wn are float64 products."""
    if ix.dtype == torch.float32:
        fin, x0, y0, w, n = UW._taps(ix, iy, H, W)
    else:
        fin = torch.isfinite(ix) & torch.isfinite(iy)
        x, y = torch.where(fin, ix, torch.zeros_like(ix)), torch.where(fin, iy, torch.zeros_like(iy))
        xf, yf = torch.floor(x), torch.floor(y)
        w, n, x0, y0 = x - xf, y - yf, xf.clamp(-2, W + 1).long(), yf.clamp(-2, H + 1).long()
    out = []
    for dx, dy, wt in ((0, 0, (1 - w) * (1 - n)), (1, 0, w * (1 - n)), (0, 1, (1 - w) * n), (1, 1, w * n)):
        xx, yy = x0 + dx, y0 + dy
        inside = fin & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        out.append((inside, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1), wt))
    return out


def _gather64(s2, taps):
    """s2 [C,HW] float64, taps of _tap_list -> [C,d,HW]: the zeros-padded bilinear value (util_warps.bilinear64's sum), differentiable in s2."""
    C = s2.shape[0]
    out = 0
    for inside, idx, wt in taps:
        val = s2[:, idx.reshape(-1)].reshape(C, *idx.shape)
        out = out + torch.where(inside.unsqueeze(0), val * wt.unsqueeze(0), torch.zeros((), dtype=s2.dtype, device=s2.device))
    return out


def exact64_grads(b, gup, sigma, metric, dev="cpu", positions=None, block=1 << 25):
    """The float64 reference of the sweep backward AT THE float32 SAMPLE POSITIONS (case_positions; `positions` replaces them, float32
    or float64 [B,V,D,HW]), and per element the quantities of the bound of this module's criterion (pin_bound).

    ref and src are float64 leaves; each view is gathered with the sum of util_warps.bilinear64 (taps outside the image and
    positions that are not finite count as zero), the cost is the reference's sum_v dist / sigma, and (cost * gup).sum() is
    differentiated by autograd.  The work goes view by view and, where a view's [C,D,HW] block exceeds `block` elements, by runs
    of planes.  Per sample (item, view, plane, pixel, channel): c = (2 | 1) / |sigma|, w_t the in-bounds taps' weights,
    S = sum_t w_t |s_t|, e = sum_t w_t s_t - r.  Summed over the samples that reach an element (autograd of the gather with these
    as upstream gradients for src, plain sums with w_t = 1 for ref):
        A0 = sum |g| c w_t |e|   (L1: |e| -> 1),      A1 = sum |g| c w_t S   (L2 only),      n = the in-bounds contributions
    (ref: n = V D), and for L1 the allowance: a sample with S > 0 and |e| <= 7 eps32 S may take another branch of sign() in fp32
    and moves g_ref by up to 2 |g| / |sigma| and g_src by 2 |g| w_t / |sigma| at its taps.
    -> dict of float64 tensors on `dev`: g_ref, g_src; A0_ref, A1_ref, n_ref, allow_ref [B,C,H,W]; A0_src, A1_src, allow_src
    [B,V,C,H,W], n_src [B,V,1,H,W]; Mb [B] (the bound M_b of csrc/sweep_bwd_det.hip on a contribution) and N = D H W."""
    dt = torch.float64
    L2 = metric == "L2"
    ref = b["ref"].to(dev, dt).detach().clone().requires_grad_(True)
    src = b["src"].to(dev, dt).detach().clone().requires_grad_(True)
    B, V, C, H, W = src.shape
    HW = H * W
    ix, iy = case_positions(b) if positions is None else positions
    ix, iy = ix.to(dev), iy.to(dev)
    D = ix.shape[2]
    g = gup.to(dev, dt).reshape(B, D, HW)
    c = (2.0 if L2 else 1.0) / abs(float(sigma))
    q = {k: torch.zeros(B, C, HW, dtype=dt, device=dev) for k in ("A0_ref", "A1_ref", "allow_ref")}
    q.update({k: torch.zeros_like(src) for k in ("A0_src", "A1_src", "allow_src")})
    q["n_src"] = torch.zeros(B, V, 1, HW, dtype=dt, device=dev)
    step = max(1, min(D, block // (C * HW)))
    for i in range(B):
        rf = ref[i].reshape(C, 1, HW)
        for v in range(V):
            for k0 in range(0, D, step):
                taps = _tap_list(ix[i, v, k0:k0 + step], iy[i, v, k0:k0 + step], H, W)
                for inside, idx, _ in taps:
                    q["n_src"][i, v, 0].index_add_(0, idx.reshape(-1), inside.reshape(-1).to(dt))
                val = _gather64(src[i, v].reshape(C, HW), taps)                       # [C,d,HW]
                gk = g[i, k0:k0 + step]
                with torch.no_grad():
                    S = _gather64(src[i, v].detach().abs().reshape(C, HW), taps)
                    e = val.detach() - rf.detach()
                    ga = (gk.abs() * c).unsqueeze(0)                                       # |g| c  [1,d,HW]
                    ups = {"A0": ga * e.abs() if L2 else ga.expand_as(e)}
                    if L2:
                        ups["A1"] = ga * S
                    else:
                        ups["allow"] = ((S > 0) & (e.abs() <= 7 * EPS32 * S)).to(dt) * (2 * ga)
                    for k, up in ups.items():
                        q[k + "_ref"][i] += up.sum(1)
                for k, up in ups.items():
                    q[k + "_src"] += torch.autograd.grad(val, src, up.contiguous(), retain_graph=True)[0]
                diff = val - rf
                dist = (diff ** 2).sum(0) if L2 else diff.abs().sum(0)
                ((dist / sigma) * gk).sum().backward()
    out = {k: (t if t.shape == src.shape else t.reshape(t.shape[:-1] + (H, W))) for k, t in q.items()}
    out.update(g_ref=ref.grad, g_src=src.grad, n_ref=torch.full_like(out["A0_ref"], float(V * D)), N=D * HW)
    gscale = abs(float(np.float32(2.0 if L2 else 1.0) / np.float32(sigma)))
    E = b["src"].abs().amax(dim=(1, 2, 3, 4)).double() + b["ref"].abs().amax(dim=(1, 2, 3)).double() if L2 else torch.ones(B, dtype=dt)
    out["Mb"] = (gscale * gup.abs().reshape(B, -1).amax(1).double().cpu() * E.cpu()).to(dev)
    return out


def pin_bound(x, which, det=False):
    """The bound of |g32 - g64| per element of g_ref / g_src (`which` = 'ref' | 'src') from the dict of exact64_grads:
    eps32 (7 A1 + (8 + n) A0) + the L1 allowance; det: + the quantisation term of the integer sum, n N M_b 2^-59 (g_src only).
    Exactly 0 where nothing contributes (A0 == A1 == 0 and no allowance)."""
    A0, A1, n, allow = (x[k + "_" + which] for k in ("A0", "A1", "n", "allow"))
    bound = EPS32 * (7 * A1 + (8 + n) * A0) + allow
    if det:
        assert which == "src"
        quant = n * (x["N"] * 2.0 ** -59) * x["Mb"].reshape(-1, 1, 1, 1, 1)
        bound = torch.where(bound > 0, bound + quant, bound)   # (no contribution, or only zeros: the integer sum is exactly 0 too)
    return bound


def pin_check(got, x, which, what, det=False, bound=None, want=None):
    """Every element of `got` within the bound of the float64 reference, exactly 0 where the bound is 0 (a texel no tap reaches
    among them).  Prints and returns the worst error / bound."""
    want = x["g_" + which] if want is None else want
    bound = pin_bound(x, which, det) if bound is None else bound
    got = got.detach().to(want.device, torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    zero = bound == 0
    assert bool((got[zero] == 0).all()), "%s: an element nothing contributes to is not exactly 0" % what
    err = (got - want).abs()
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    note = ""
    if bool((x["allow_" + which] > 0).any()):   # L1: an element with an allowance may sit at a whole sign flip; the others for the record
        plain = ~zero & (x["allow_" + which] == 0)
        note = " (%.4f over the elements without an L1 allowance)" % float((err[plain] / bound[plain]).max())
    print("%s: worst error / bound = %.4f%s; max error %.3e of max |g64| %.3e; %d of %d elements exactly 0"
          % (what, ratio, note, float(err.max()), float(want.abs().max()), int(zero.sum()), zero.numel()))
    bad = err > bound
    if bool(bad.any()):
        at = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d elements outside the bound, worst error / bound = %.4f, first at %s" % (what, int(bad.sum()), ratio, at))
    return ratio


def allowance_share(x):
    """(share of g_ref's, of g_src's elements that carry a non-zero L1 allowance)."""
    return tuple(float((x["allow_" + w] > 0).double().mean()) for w in ("ref", "src"))


def max_err(g, x, which):
    """max over the elements of (|g - g64| - the L1 allowance)+ : the figure of the project's max-norm rule
    max|g - g64| <= 2 E_ref + eps32 max|g64|, E_ref the same figure of the CPU fp32 autograd of oracle_cost."""
    want = x["g_" + which]
    d = (g.detach().to(want.device, torch.float64) - want).abs() - x["allow_" + which]
    return float(d.clamp_min(0).max())


# ---- the plane groups of the g_src pass, restated on the host ------------------------------------------------------------
def kernel_constants():
    """(BOX_CAP, BT) as csrc/sweep_bwd_body.hpp declares them: the cases below are chosen against these two numbers."""
    text = open(KERNEL).read()
    found = []
    for name in ("BOX_CAP", "BT"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, "csrc/sweep_bwd_body.hpp no longer declares 'constexpr int %s = <number>;'" % name
        found.append(int(m.group(1)))
    return tuple(found)


_BIG = 1 << 30


def plane_boxes(ix, iy, H, W, tile):
    """Per plane and tile, the box of the in-bounds taps of the tile's live pixels: (x_lo, x_hi, y_lo, y_hi), each an int64
    array [D, tiles_y, tiles_x]; no in-bounds tap: x_lo > x_hi.  A tap is one of the four texels (floor(ix) + {0, 1},
    floor(iy) + {0, 1}); it is in bounds when it lies in [0, W) x [0, H) and the position is finite."""
    ix, iy = np.asarray(ix, dtype=np.float32).reshape(-1, H, W), np.asarray(iy, dtype=np.float32).reshape(-1, H, W)
    finite = np.isfinite(ix) & np.isfinite(iy)
    with np.errstate(invalid="ignore"):
        x0 = np.clip(np.floor(np.where(finite, ix, -2.0)), -2, W + 1).astype(np.int64)   # (beyond -2 / size + 1: out anyway)
        y0 = np.clip(np.floor(np.where(finite, iy, -2.0)), -2, H + 1).astype(np.int64)
    xin0, xin1 = finite & (x0 >= 0) & (x0 < W), finite & (x0 + 1 >= 0) & (x0 + 1 < W)
    yin0, yin1 = finite & (y0 >= 0) & (y0 < H), finite & (y0 + 1 >= 0) & (y0 + 1 < H)
    any_x, any_y = xin0 | xin1, yin0 | yin1
    lo_hi = (np.where(xin0 & any_y, x0, np.where(xin1 & any_y, x0 + 1, _BIG)),
             np.where(xin1 & any_y, x0 + 1, np.where(xin0 & any_y, x0, -_BIG)),
             np.where(yin0 & any_x, y0, np.where(yin1 & any_x, y0 + 1, _BIG)),
             np.where(yin1 & any_x, y0 + 1, np.where(yin0 & any_x, y0, -_BIG)))
    ty, tx = -(-H // tile), -(-W // tile)
    out = []
    for j, a in enumerate(lo_hi):
        fill = _BIG if j % 2 == 0 else -_BIG
        pad = np.full((a.shape[0], ty * tile, tx * tile), fill, dtype=np.int64)
        pad[:, :H, :W] = a
        pad = pad.reshape(-1, ty, tile, tx, tile)
        out.append(pad.min(axis=(2, 4)) if j % 2 == 0 else pad.max(axis=(2, 4)))
    return tuple(out)


def _union(u, box):
    return (min(u[0], box[0]), max(u[1], box[1]), min(u[2], box[2]), max(u[3], box[3]))


def box_area(box):
    return (box[1] - box[0] + 1) * (box[3] - box[2] + 1) if box[0] <= box[1] else 0


def group_planes(boxes, cap):
    """The groups of one (tile, view) pair from its per-plane boxes, greedy as the kernel forms them: extend the group while
    the union of the boxes has at most `cap` texels (a plane with no in-bounds tap adds nothing to the union).
    -> list of ("staged", k0, k1, box), ("direct", k, box) -- a plane whose own box exceeds the cap --, ("empty", k0, k1):
    planes k0 <= k < k1, box = (x_lo, x_hi, y_lo, y_hi) inclusive."""
    none = (_BIG, -_BIG, _BIG, -_BIG)
    out, k, D = [], 0, len(boxes)
    while k < D:
        u, k1 = none, k
        while k1 < D:
            n = _union(u, boxes[k1])
            if box_area(n) > cap:
                break
            u, k1 = n, k1 + 1
        if k1 == k:
            out.append(("direct", k, tuple(int(x) for x in boxes[k])))
            k1 = k + 1
        elif u[0] <= u[1]:
            out.append(("staged", k, k1, tuple(int(x) for x in u)))
        else:
            out.append(("empty", k, k1))
        k = k1
    return out


def tile_groups(b, cap, tile):
    """{(item, view, tile_y, tile_x): groups (see group_planes)} for a batch dict of synth.make_batch: what the g_src pass of
    csrc/sweep_bwd.hip does with every (tile, view) pair, from the sample positions of oracle.ref_cpu.sample_coords."""
    B, V, C, H, W = b["src"].shape
    out = {}
    for i in range(B):
        K = b["K"][i]
        cx, cy = K.numpy()[0, 2], K.numpy()[1, 2]
        for v in range(V):
            ix, iy = O.sample_coords(K, b["R"][i, v], b["t"][i, v], b["rays"][i], b["d_candi"], cx, cy, H, W)
            x_lo, x_hi, y_lo, y_hi = plane_boxes(ix.numpy(), iy.numpy(), H, W, tile)
            for ty in range(x_lo.shape[1]):
                for tx in range(x_lo.shape[2]):
                    boxes = [(x_lo[k, ty, tx], x_hi[k, ty, tx], y_lo[k, ty, tx], y_hi[k, ty, tx]) for k in range(x_lo.shape[0])]
                    out[(i, v, ty, tx)] = group_planes(boxes, cap)
    return out


def pair_box(groups):
    """The union of the boxes of a pair's staged groups and direct planes, or None."""
    u = (_BIG, -_BIG, _BIG, -_BIG)
    for g in groups:
        if g[0] != "empty":
            u = _union(u, g[-1])
    return u if u[0] <= u[1] else None


def describe(groups):
    def one(g):
        if g[0] == "staged":
            return "staged[%d:%d] x %d..%d y %d..%d (%d texels)" % (g[1], g[2], *g[3], box_area(g[3]))
        if g[0] == "direct":
            return "direct[%d] x %d..%d y %d..%d (%d texels)" % (g[1], *g[2], box_area(g[2]))
        return "empty[%d:%d]" % (g[1], g[2])
    return ", ".join(one(g) for g in groups)


def group_stats(tg, C, channels_per_pass=4):
    """The counts that the coverage test holds the cases to."""
    kinds = {key: [g[0] for g in gs] for key, gs in tg.items()}
    follows = sum(1 for ks in kinds.values() for a, b_ in zip(ks, ks[1:]) if a == "empty" and b_ in ("direct", "staged"))
    return {"pairs": len(tg),
            "staged": sum(ks.count("staged") for ks in kinds.values()),
            "direct": sum(ks.count("direct") for ks in kinds.values()),
            "direct_with_channel_tail": sum(ks.count("direct") for ks in kinds.values()) if C % channels_per_pass else 0,
            "pairs_3_groups": sum(1 for ks in kinds.values() if len(ks) >= 3),
            "pairs_split_no_direct": sum(1 for ks in kinds.values() if ks.count("staged") >= 2 and "direct" not in ks),
            "pairs_all_empty": sum(1 for ks in kinds.values() if set(ks) == {"empty"}),
            "empty_then_group": follows}


def _zoom_case(config_id, C, H, W, V, d_lo, d_hi, ts, B=1, roll_deg=None):
    """make_batch(..., D = 16, pose 'mono') with R, t and d_candi overwritten: R = a roll about the optical axis (identity
    without one), t as given per (item, view).  min(d_candi) + t_z >= 1: no plane comes near the camera plane."""
    b = synth.make_batch(config_id, B, C=C, D=16, H=H, W=W, V=V, pose="mono")
    b["d_candi"] = synth.powerf(d_lo, d_hi, 16, 1.0)
    t = torch.tensor(ts, dtype=torch.float32).reshape(B, V, 3)
    assert float(b["d_candi"].min() + t[..., 2].min()) >= 1.0
    R = torch.eye(3).repeat(B, V, 1, 1)
    if roll_deg is not None:
        for i in range(B):
            for v in range(V):
                a = np.deg2rad(roll_deg[i][v])
                R[i, v] = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    b["R"], b["t"] = R, t
    return b


def group_cases():
    """name -> batch dict.  The source camera stands in FRONT of the reference one (t_z < 0), so the warp magnifies: the taps
    of a 16 x 16 tile of near planes spread over more texels than the LDS box image holds.

    A: 72 x 88 (ragged in both directions: 8 live rows and columns in the last tiles), C = 11 (3 live channels in the second
       channel pass).  View 0 zooms 5x on the nearest plane, 1.5x on the farthest; the tile that holds the principal point
       spreads into all four quadrants and goes over the cap.  View 1 is a lateral baseline that pushes whole tiles out of
       the image.
    C: 88 x 104, one view, a milder zoom: a pair splits into two staged groups, no direct plane.
    E: 72 x 120, one view, planes 5 ... 20 m apart by 1 m: the lateral baseline throws the nearest plane of the leftmost middle
       tile out of the image altogether and the next one back into it at 3x, whole: an empty run, then a direct plane.
    R: two items of two views, 80 x 120, each view rolled about the optical axis by another angle: the boxes of a rolled
       tile are wider than the tile's footprint, more pairs split, and the second item's outputs lie behind the first's."""
    return {
        "A": _zoom_case(41, 11, 72, 88, 2, 5.0, 12.0, [[(0.3, 0.1, -4.0), (9.0, 0.0, 0.5)]]),
        "C": _zoom_case(42, 5, 88, 104, 1, 4.0, 10.0, [[(0.5, 0.2, -2.6)]]),
        "E": _zoom_case(44, 11, 72, 120, 1, 5.0, 20.0, [[(5.2, -0.2, -4.0)]]),
        "R": _zoom_case(43, 9, 80, 120, 2, 5.0, 12.0, [[(0.3, 0.1, -3.5), (-0.4, 0.2, -2.0)], [(6.0, -0.3, -3.0), (0.0, 0.0, -4.0)]],
                        B=2, roll_deg=[[35.0, -20.0], [10.0, 45.0]]),
    }
