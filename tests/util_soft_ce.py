"""Shared by tests/test_soft_ce_host.py and tests/test_soft_ce_gpu.py: a float64 restatement of the soft-label cross-entropy
(ops.dpv_soft_ce; csrc/loss.hip: soft_ce_vec4_kernel<FROM_DEPTH,RPL>, soft_ce_scalar_kernel<FROM_DEPTH>, soft_ce_final_kernel and
the two backward kernels), per pixel and per item, forward and backward, the a-priori per-element bounds a float32 evaluation of
it is held to, a restatement of the dispatch (which_path), float32 emulations of the kernels' two summation orders, twelve
mistakes the bounds must catch, and the input families.

The operation, on the float32 inputs exactly as given (v = logp, d = d_candi, m = mask, z = depth_gt), per item b and pixel p:
    ce[b,p]    = - sum_k label[b,k,p] v[b,k,p]
    loss[b]    = sum_{p: m != 0} ce[b,p] m[b,p] / count[b],  count[b] = #{p: m[b,p] == 1}; 0 where count[b] == 0; without a mask
                 the mean over all H W pixels.  A pixel with m == 0 is skipped, not multiplied: a NaN or inf behind it stays there.
    depth[b,p] = sum_k d_k exp(v[b,k,p])
    g_logp[b,k,p] = c label[b,k,p] + (g_depth[b,p] d_k) exp(v[b,k,p]),  c = -(g_loss[b] m / count[b]) where count[b] > 0 and
                 m != 0, else 0 (and the first term is exactly 0 where c is 0, whatever the label holds)
The label is read (it may hold -1, or anything else) or formed from z: with sigma = sqrt(variance), den = 2 sigma^pow,
    arg_k = |d_k - z|^pow / den,  g_k = exp(-arg_k),  S = sum_k g_k,  label_k = g_k / S,  and -1 on every plane where S is 0 or NaN
so that ce = -(sum_k g_k v_k) / S, or sum_k v_k under the -1 label.  variance and pow are rounded to float32 first, as the C entry
receives them.  No term is skipped in the sums: 0 * -inf = NaN falls out of the arithmetic as it does out of label * logp.

The -1 label and the band.  float32 loses S to underflow where float64 does not, so the restatement decides the -1 label from
S64: -1 where not S64 > 2^-116, normalised above.  Below 2^-160 every g_k is under 2^-11 of the smallest float32 denormal and
expf gives 0 on every plane, S32 = 0; above 2^-116 one g_k is at least 2^-116 / 128 = 2^-123, a normal float32, S32 > 0.  In
between neither precision is right, and that is a condition on the inputs: depth_maps() redraws every pixel whose S64 lies in
[2^-160, 2^-116], reference() refuses inputs that have one, and no comparison leaves anything out.

The bounds (bound()).  u = 2^-24, gamma_n = n u / (1 - n u).  The library is built with -ffp-contract=off: every product and
every sum rounds once.  n is the longest chain of additions behind a pixel: ceil(D / 4) + 2 on the vec4 kernels (the planes of one
lane in ascending order, then the two adds of group_sum), D on the scalar kernels and for a float32 sum in any order ("any": every
term passes at most D - 1 additions and its own product).  A denormal (or flushed) intermediate costs at most 2^-126 per
operation; that is the absolute floor F 2^-126 added to every bound, F = D + 4 for ce and depth (D products or exps, the adds
above them being exact on denormals), D + 20 for loss (ce's, then 11 levels and 3 final operations, rounded up), 8 for g_logp.
  ce, label form      |ce^ - ce| <= gamma_(n+1) sum_k |label_k v_k|
  depth               |e^ - e|   <= (gamma_(n+1) + e_exp u) sum_k |d_k| exp(v_k)
  loss                a workgroup adds ce m (one product) through (w0 + w1) + (w2 + w3) in a lane and the 8 levels of wg_sum_put /
                      wg_sum_get: k = 11 roundings at most (the scalar kernel: 9).  The partial sums are added in float64 (nothing
                      at this scale), converted to float (u) and divided by count (u):
                      E = [(1 + gamma_k) sum_p |m| E_ce + gamma_k sum_p |ce m|] / count,   E_loss = E + 3 u (|loss| + E)
                      ("any": k = H W + 1).  count is exact.
  g_logp, label form  c label is -((g_loss m) / count) label: three roundings of a product chain, gamma_3 |c label| and no absolute
                      term.  With a depth gradient t = (g_depth d_k) expf(v) has two roundings and expf's error, and the sum
                      rounds once more: gamma_4 |c label| + (gamma_3 + e_exp u)(1 + gamma_4) |t|.
  from-depth form     a^ = |d_k - z| (u); p^ = a^ a^ (3 u in all) or powf(a^, pow) (pow u from a^, e_pow u from powf); den^ against
                      the exact 2 sigma^pow: sqrtf (u), then sig sig (3 u in all) or the host's powf, taken at its documented 1 ulp
                      <= 2 u ((pow + 2) u in all); the division (u).  So arg^ = arg (1 + theta), |theta| <= A u with
                      A = 3 + 3 + 1 = 7 for pow == 2 and A = (pow + e_pow) + (pow + 2) + 1 otherwise, and
                          g^_k = g_k exp(-arg_k theta)(1 + e_exp u'):  |g^_k - g_k| <= rho_k g_k,  rho_k = expm1(A arg_k u) + e_exp u
                      plus, where g_k < 2^-125, the whole of it and two denormal steps (t_k = g_k + 2^-148: expf's result is
                      rounded to a denormal or flushed).  E_g = rho_k g_k + t_k.  With n as above
                          E_S   = sum_k E_g + gamma_n sum_k (g_k + E_g),                eps_S = E_S / S
                          E_num = sum_k E_g |v_k| + gamma_(n+1) sum_k (g_k + E_g) |v_k|
                          num^/S^ - num/S = (num^ - num)/S^ - num (S^ - S)/(S S^):
                          E_ce  = (E_num + |ce| E_S) / (S (1 - eps_S)), then the division rounds: + u (|ce| + E_ce)
                      and under the -1 label ce = sum_k v_k: gamma_n sum_k |v_k|.  The label of the backward is g^_k / S^ (u):
                          E_lab = label_k (rho_k + eps_S / (1 - eps_S) + u)(1 + eps_S) + t_k / (S (1 - eps_S)),   0 under the -1 label
                          E_g_logp = |c| E_lab (1 + gamma_3) + gamma_3 |c label| (+ the depth term as above)
Where the reference is not finite the result must be of its class (NaN, +inf, -inf): util_correlation.ratio.

The two device-function errors.  The ROCm toolkit this was written against ships no HIP math documentation, so both were measured
on an MI355X against float64 exp / pow, relative error of a normal result in units of u, over the arguments this suite produces:
    expf   x in [-87.33, 0] (every argument with a normal result; 2^24 uniform, 2^24 in [-1, 0], 2^24 log-uniform):  1.411 u
    powf   a in (0, 64] and [2^-24, 64] (2^24 uniform and 2^24 log-uniform each), pow 1, 3, 0.5:  1.999, 2.300, 2.311 u
A sample does not see the worst argument: the bounds use twice the largest, e_exp = 2.83 and e_pow = 4.63.  Nothing here was
tuned against dpv_soft_ce's own output.

Which kernel a call runs (which_path restates launch_dpv_soft_ce and launch_dpv_soft_ce_backward of csrc/loss.hip):
    H W % 4 == 0, D <= 128 and every pointer passed 16-byte aligned:  vec8 | vec16 | vec32 for D <= 32 | 64 | 128 (for_planes_per_lane)
    otherwise:                                                        scalar
The pointers are those of the tensors the binding passes, data_ptr() after .contiguous(): logp, label or depth_gt, mask, and in
the backward g_depth; the outputs (depth, g_logp) are fresh allocations, aligned.
"""
import math

import torch

from util_correlation import classes, ratio, worst  # noqa: F401  (the comparison by class is the correlation suite's)

U32 = 2.0 ** -24
TINY32 = 2.0 ** -126
E_EXP, E_POW = 2.83, 4.63      # of the device expf / powf, in u: twice the measured 1.411 / 2.311 (module docstring)
BAND_LO, BAND_HI = 2.0 ** -160, 2.0 ** -116
VEC = {8: "vec8", 16: "vec16", 32: "vec32"}
SCALAR = "scalar"


# ---- dispatch ------------------------------------------------------------------------------------------------------------------
def planes_per_lane(D):
    assert D <= 128
    return 8 if D <= 32 else 16 if D <= 64 else 32


def which_path(shape, tensors):
    """"vec8" | "vec16" | "vec32" | "scalar" for a call on a [B,D,H,W] volume that passes `tensors` (None entries are absent)."""
    B, D, H, W = shape
    ptrs = [t.data_ptr() for t in tensors if t is not None]
    assert all(t.is_contiguous() for t in tensors if t is not None)
    if (H * W) % 4 == 0 and D <= 128 and all(p % 16 == 0 for p in ptrs):
        return VEC[planes_per_lane(D)]
    return SCALAR


def chain(D, path):
    """The longest chain of additions behind one pixel's sum over D."""
    return -(-D // 4) + 2 if path in VEC.values() else D


def tree(HW, path):
    """Roundings between a pixel's ce and its workgroup's partial sum."""
    return HW + 1 if path == "any" else 11


def gamma(n):
    assert n * U32 < 0.01
    return n * U32 / (1 - n * U32)


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
MUTANTS = {   # name: (the output it corrupts, the label source it needs or None for either)
    "drop_last_plane": ("ce", None),             # the plane D - 1 is left out when D % 4 != 0
    "half_group_sum": ("ce", None),              # group_sum stops after one shuffle: plane groups 2 and 3 are left out
    "wrong_pairing": ("ce", "depth"),            # plane g + 4 i takes the candidate 4 g + i
    "drop_last_quad": ("loss", None),            # the last four pixels of an item never reach the sum
    "count_nonzero": ("loss", None),             # count = #(m != 0)
    "mask_multiplied": ("loss", None),           # a masked-out pixel is multiplied by 0 instead of skipped
    "coef_ignores_mask_value": ("g_logp", None),  # c = -(g_loss / count) wherever m != 0
    "minus_one_gives_zero": ("ce", "depth"),     # the fallback label is 0 instead of -1
    "den_is_variance": ("ce", "depth"),          # den = variance instead of 2 sigma^pow
    "pow_ignored": ("ce", "depth"),              # always the square
    "not_normalised": ("ce", "depth"),           # g_k instead of g_k / S
    "gdepth_uses_v": ("g_logp", None),           # (g_depth d_k) v instead of (g_depth d_k) exp(v)
}


def f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def in_band(S64):
    return (S64 >= BAND_LO) & (S64 <= BAND_HI)


def gauss64(dc, z, variance, pow):
    """arg [B,D,H,W] = |d_k - z|^pow / (2 sqrt(variance)^pow) in float64 from float32 d_candi [D], depth_gt [B,H,W]."""
    pw, var = f32(pow), f32(variance)
    a = (dc.double().view(1, -1, 1, 1) - z.double().unsqueeze(1)).abs()
    return (a * a if pw == 2.0 else a ** pw) / (2.0 * math.sqrt(var) ** pw)


def reference(logp, dc, label=None, depth_gt=None, variance=None, pow=2.0, mask=None, g_loss=None, g_depth=None, mutant=None):
    """dict in float64 from float32 host tensors: ce, depth [B,H,W]; count, loss [B]; label [B,D,H,W] (read or formed), minus
    [B,H,W] (the -1 set of the from-depth form); g_logp [B,D,H,W] with its two terms t1, t2 and c when a gradient is given; the
    magnitudes A_ce = sum_k |label v|, A_loss = sum_p |ce m|, A_depth = sum_k |d_k| exp(v) and, from depth, g, S, arg."""
    assert mutant is None or mutant in MUTANTS
    assert (label is None) != (depth_gt is None)
    v = logp.double()
    B, D, H, W = v.shape
    d = dc.double().view(1, D, 1, 1)
    keep = torch.ones(D, dtype=torch.bool)
    if mutant == "drop_last_plane" and D % 4:
        keep[D - 1] = False
    if mutant == "half_group_sum":
        keep = (torch.arange(D) % 4) < 2
    kp = keep.view(1, D, 1, 1)
    zero = torch.zeros((), dtype=torch.float64)
    pick = lambda t: torch.where(kp, t, zero)
    r = {"form": "label" if label is not None else "depth", "D": D, "HW": H * W, "pow": f32(pow), "v": v}
    if label is not None:
        lab = label.double()
        ce = -pick(lab * v).sum(1)
        r.update(A_ce=pick((lab * v).abs()).sum(1), minus=torch.zeros(B, H, W, dtype=torch.bool))
    else:
        pw, var = f32(pow), f32(variance)
        dk = d
        if mutant == "wrong_pairing":
            k = torch.arange(D)
            dk = d[:, (4 * (k % 4) + k // 4) % D]
        a = (dk - depth_gt.double().unsqueeze(1)).abs()
        p = a * a if (pw == 2.0 or mutant == "pow_ignored") else a ** pw
        arg = p / (var if mutant == "den_is_variance" else 2.0 * math.sqrt(var) ** pw)
        g = torch.exp(-arg)
        S = pick(g).sum(1)
        if mutant is None:
            assert not bool(in_band(S).any()), "depth_gt has pixels whose S64 is inside the band: redraw them (depth_maps)"
        minus = ~(S > BAND_HI)
        Sn = torch.ones_like(S) if mutant == "not_normalised" else S
        fallback = 0.0 if mutant == "minus_one_gives_zero" else -1.0
        ce = torch.where(minus, -fallback * pick(v).sum(1), -(pick(g * v).sum(1) / Sn))
        lab = torch.where(minus.unsqueeze(1), torch.full_like(g, fallback), g / Sn.unsqueeze(1))
        r.update(A_ce=torch.where(minus, pick(v.abs()).sum(1), pick(g * v.abs()).sum(1) / Sn), minus=minus, g=g, S=S, arg=arg)
    e = torch.exp(v)
    r.update(ce=ce, label=lab, depth=pick(d * e).sum(1), A_depth=pick(d.abs() * e).sum(1))
    # the mean over the mask
    m = torch.ones(B, H, W, dtype=torch.float64) if mask is None else mask.double()
    valid = m != 0
    w = ce * m if mutant == "mask_multiplied" else torch.where(valid, ce * m, zero)
    one = (m != 0) if mutant == "count_nonzero" else (m == 1)
    if mutant == "drop_last_quad":
        w, one = w.clone(), one.clone()
        w.view(B, -1)[:, -4:] = 0
        one.view(B, -1)[:, -4:] = False
    count = one.sum((1, 2)).double()
    loss = torch.where(count > 0, w.sum((1, 2)) / count.clamp(min=1), zero)
    r.update(m=m, count=count, loss=loss, A_loss=w.abs().sum((1, 2)))
    # the gradient
    if g_loss is not None or g_depth is not None:
        gl = torch.zeros(B, dtype=torch.float64) if g_loss is None else g_loss.double()
        mm = torch.ones_like(m) if mutant == "coef_ignores_mask_value" else m
        c = torch.where((count > 0).view(B, 1, 1) & valid, -(gl.view(B, 1, 1) * mm / count.clamp(min=1).view(B, 1, 1)), zero)
        c4 = c.unsqueeze(1)
        t1 = torch.where(c4 != 0, c4 * lab, zero)
        t2 = torch.zeros_like(t1)
        if g_depth is not None:
            t2 = (g_depth.double().unsqueeze(1) * d) * (v if mutant == "gdepth_uses_v" else e)
        r.update(c=c, t1=t1, t2=t2, g_logp=t1 + t2, has_gd=g_depth is not None)
    return r


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def arg_coef(pw):
    """A of the module docstring: arg^ = arg (1 + theta), |theta| <= A u."""
    return 7.0 if pw == 2.0 else (pw + E_POW) + (pw + 2.0) + 1.0


def bound(r, path):
    """dict(ce, depth, loss[, g_logp]) of per-element bounds (float64) on a float32 evaluation of reference() r in the order of
    `path` (vec8 | vec16 | vec32 | scalar | any); NaN or inf where the reference is not finite (the class is compared there)."""
    D, v = r["D"], r["v"]
    n = chain(D, path)
    zero = torch.zeros((), dtype=torch.float64)
    if r["form"] == "label":
        E_ce = gamma(n + 1) * r["A_ce"]
    else:
        g, S, arg, minus = r["g"], r["S"], r["arg"], r["minus"]
        rho = torch.expm1(arg_coef(r["pow"]) * arg * U32) + E_EXP * U32
        t = torch.where(g < 2.0 ** -125, g + 2.0 ** -148, zero)
        Eg = torch.where(g > 0, rho * g, zero) + t
        ES = Eg.sum(1) + gamma(n) * (g + Eg).sum(1)
        eps = ES / S
        EN = (Eg * v.abs()).sum(1) + gamma(n + 1) * ((g + Eg) * v.abs()).sum(1)
        E = (EN + r["ce"].abs() * ES) / (S * (1 - eps))
        E = E + U32 * (r["ce"].abs() + E)
        E_ce = torch.where(minus, gamma(n) * v.abs().sum(1), E)
        assert bool((eps[~minus] < 0.5).all())
        eps4, S4 = eps.unsqueeze(1), S.unsqueeze(1)
        E_lab = r["label"].abs() * (rho + eps4 / (1 - eps4) + U32) * (1 + eps4) + t / (S4 * (1 - eps4))
        E_lab = torch.where(minus.unsqueeze(1), zero, E_lab)
    E_ce = E_ce + (D + 4) * TINY32
    out = {"ce": E_ce, "depth": (gamma(n + 1) + E_EXP * U32) * r["A_depth"] + (D + 4) * TINY32}
    if r["form"] == "depth":
        out["label"] = E_lab + TINY32
    k = tree(r["HW"], path)
    m, cnt = r["m"], r["count"].clamp(min=1)
    EE = torch.where(m != 0, m.abs() * E_ce, zero).sum((1, 2))
    E = ((1 + gamma(k)) * EE + gamma(k) * r["A_loss"]) / cnt
    out["loss"] = torch.where(r["count"] > 0, E + 3 * U32 * (r["loss"].abs() + E), zero) + (D + 20) * TINY32
    if "g_logp" in r:
        c = r["c"].unsqueeze(1).abs()
        E1 = gamma(4 if r["has_gd"] else 3) * r["t1"].abs()
        if r["form"] == "depth":
            E1 = E1 + torch.where(c != 0, c * E_lab * (1 + gamma(3)), zero)
        out["g_logp"] = E1 + (gamma(3) + E_EXP * U32) * (1 + gamma(4)) * r["t2"].abs() + 8 * TINY32
    return out


def probe_bound(r, E_ce, path):
    """The bound on loss[b] of the probe batch: item b's mask is 1 at pixel b alone, so loss[b] = ce[b] / 1 through the same tree."""
    k = tree(r["HW"], path)
    E = (1 + gamma(k)) * E_ce + gamma(k) * r["ce"].abs()
    return E + 3 * U32 * (r["ce"].abs() + E) + (r["D"] + 20) * TINY32


# ---- input families ---------------------------------------------------------------------------------------------------------------
PROBE_D = (1, 3, 4, 5, 32, 33, 64, 65, 100, 127, 128)   # D = 3 leaves a plane group empty; the first and a ragged D of every class
PROBE_HW = ((9, 12), (13, 20))                          # 108 pixels: less than a workgroup; 260: the second holds one live quad
SCALAR_HW = ((7, 9), (1, 257))                          # H W % 4 != 0: 63 pixels, and two workgroups
SCALAR_D = (129, 130)                                   # D > 128, at 8 x 8
DEPTH_FORMS = ((0.3, 2.0), (0.3, 1.0), (0.3, 3.0), (0.3, 0.5), (0.01, 2.0))   # (variance, pow) of the from-depth cases
VOLUMES = ("soft2", "soft12", "peaked")
MASKS = ("binary", "values", "zero_item", "none")
NONFINITE = ("nonfinite", "nonfinite_masked")


def candidates(D):
    return torch.linspace(5.0, 40.0, D)


def volume(kind, shape, g):
    """soft2 / soft12: log_softmax of 2 or 12 N(0,1) over D + 1 planes, the first D of them (so that D = 1 is not all zeros);
    peaked: one plane within 1e-3 of 0, the others -40 + N(0,1)."""
    B, D, H, W = shape
    if kind == "peaked":
        x = -40.0 + torch.randn(B, D, H, W, generator=g, dtype=torch.float64)
        x.scatter_(1, torch.randint(0, D, (B, 1, H, W), generator=g), -1e-3 * torch.rand(B, 1, H, W, generator=g, dtype=torch.float64))
        return x.float()
    scale = {"soft2": 2.0, "soft12": 12.0}[kind]
    return torch.log_softmax(scale * torch.randn(B, D + 1, H, W, generator=g, dtype=torch.float64), 1)[:, :D].float()


def labels(shape, g):
    """softmax of 3 N(0,1), a tenth of the entries exactly 0, and one pixel of item 0 that holds -1 on every plane."""
    B, D, H, W = shape
    lab = torch.softmax(3 * torch.randn(B, D, H, W, generator=g, dtype=torch.float64), 1).float()
    lab = torch.where(torch.rand(B, D, H, W, generator=g) < 0.1, torch.zeros(()), lab)
    if H * W > 1:
        lab.view(B, D, -1)[0, :, 1] = -1.0
    return lab


def depth_maps(shape, dc, variance, pow, g, edges=True):
    """z in [4, 42] (a little beyond the candidates on both sides); with edges, pixels 2.. of every item are: exactly on a
    candidate, midway between two, below d_0 (3), above d_(D-1) (45) and far out (60).  Every pixel whose S64 is inside the band
    is drawn again."""
    B, D, H, W = shape
    z = 4.0 + 38.0 * torch.rand(B, H, W, generator=g)
    if edges and H * W >= 8:
        k = D // 2
        flat = z.view(B, -1)
        flat[:, 2] = dc[k]
        flat[:, 3] = ((dc[k].double() + dc[min(k + 1, D - 1)].double()) / 2).float()
        flat[:, 4], flat[:, 5], flat[:, 6] = 3.0, 45.0, 60.0
    for _ in range(64):
        bad = in_band(torch.exp(-gauss64(dc, z, variance, pow)).sum(1))
        if not bool(bad.any()):
            return z
        z[bad] = 4.0 + 38.0 * torch.rand(int(bad.sum()), generator=g)
    raise AssertionError("no depth map outside the band after 64 draws")


def masks(kind, shape, g):
    B, D, H, W = shape
    if kind == "none":
        return None
    m = (torch.rand(B, H, W, generator=g) < 0.6).float()
    if kind == "values":
        sel = torch.rand(B, H, W, generator=g)
        m = torch.where(sel < 0.2, torch.full_like(m, 0.5), torch.where(sel > 0.8, torch.full_like(m, 2.0), m))
    if kind == "zero_item":
        m[B - 1] = 0.0
    return m


def make_case(family, form, shape, seed, mask_kind="binary", variance=0.3, pow=2.0, edges=True):
    """dict(logp, dc, label | depth_gt (+ variance, pow), mask, g_loss, g_depth) of float32 host tensors.  family: one of VOLUMES,
    or of NONFINITE (on a soft2 volume, B >= 2): a -inf on the plane nearest the ground truth (label > 0: ce = +inf) in item 0 and,
    with a label tensor, a -inf on a plane whose label is exactly 0 (ce = NaN) in item 1 -- at pixels whose mask is 1
    (nonfinite) or 0 (nonfinite_masked: nothing leaks); or "badz" (from depth): a NaN and a +inf in depth_gt, the label is -1."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    dc = candidates(D)
    c = {"dc": dc, "logp": volume(family if family in VOLUMES else "soft2", shape, g), "variance": variance, "pow": pow,
         "label": None, "depth_gt": None, "mask": masks(mask_kind, shape, g)}
    if form == "label":
        c["label"] = labels(shape, g)
    else:
        c["depth_gt"] = depth_maps(shape, dc, variance, pow, g, edges)
    c["g_loss"] = 0.5 + torch.rand(B, generator=g)
    c["g_depth"] = torch.randn(B, H, W, generator=g)
    if family in NONFINITE:
        assert B >= 2 and H * W >= 12 and c["mask"] is not None
        p0, p1 = H * W - 3, H * W // 2
        on = 0.0 if family == "nonfinite_masked" else 1.0
        if form == "depth":
            c["depth_gt"].view(B, -1)[0, p0] = dc[D // 2] + 0.05   # (a normalised label there)
        lab =reference(c["logp"], dc, c["label"], c["depth_gt"], variance, pow)["label"]
        k0 = int(lab.view(B, D, -1)[0, :, p0].argmax())
        assert float(lab.view(B, D, -1)[0, k0, p0]) > 0
        c["logp"].view(B, D, -1)[0, k0, p0] = float("-inf")
        c["mask"].view(B, -1)[0, p0] = on
        if form == "label":
            c["label"].view(B, D, -1)[1, D // 2, p1] = 0.0
            c["logp"].view(B, D, -1)[1, D // 2, p1] = float("-inf")
            c["mask"].view(B, -1)[1, p1] = on
    elif family == "badz":
        assert form == "depth" and H * W >= 12
        c["depth_gt"].view(B, -1)[0, 7] = float("nan")
        c["depth_gt"].view(B, -1)[B - 1, 9] = float("inf")
    else:
        assert family in VOLUMES
    return c


def source(c):
    """The label source of a case as reference()'s and the bindings' keyword arguments."""
    if c["label"] is not None:
        return {"label": c["label"]}
    return {"depth_gt": c["depth_gt"], "variance": c["variance"], "pow": c["pow"]}


def case_reference(c, grads="both", mutant=None):
    gl = c["g_loss"] if grads in ("both", "loss") else None
    gd = c["g_depth"] if grads in ("both", "depth") else None
    return reference(c["logp"], c["dc"], mask=c["mask"], g_loss=gl, g_depth=gd, mutant=mutant, **source(c))


# ---- float32 emulations of the kernels' two orders, CPU only ------------------------------------------------------------------------
def _sum_over_planes(term, D, order):
    """sum_k term(k) in float32: 'vec4' = the four lane chains over the planes g + 4 i, combined as group_sum does (lane l adds
    lane l ^ 16, then lane l ^ 32: (s0 + s1) + (s2 + s3) seen from plane group 0); 'scalar' = ascending."""
    if order == "scalar":
        acc = torch.zeros_like(term(0))
        for k in range(D):
            acc = acc + term(k)
        return acc
    assert order == "vec4"
    s = []
    for grp in range(4):
        acc = torch.zeros_like(term(0))
        for k in range(grp, D, 4):
            acc = acc + term(k)
        s.append(acc)
    return (s[0] + s[1]) + (s[2] + s[3])


def _workgroup_sums(w, order):
    """[B,HW] float32 per-pixel weights -> [B,nblk] partial sums in the kernels' order: 256 pixels per workgroup, 4 waves of 64
    lanes added by xor-shuffles 32 .. 1, then (s0 + s1) + (s2 + s3).  vec4: lane q < 16 of a wave holds (w0 + w1) + (w2 + w3) of
    its quad, the other lanes 0; scalar: lane = pixel."""
    B, HW = w.shape
    nblk = (HW + 255) // 256
    pad = torch.zeros(B, nblk * 256, dtype=torch.float32)
    pad[:, :HW] = w
    if order == "vec4":
        q = pad.view(B, nblk, 4, 16, 4)
        lanes = torch.zeros(B, nblk, 4, 64, dtype=torch.float32)
        lanes[..., :16] = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    else:
        lanes = pad.view(B, nblk, 4, 64).clone()
    idx = torch.arange(64)
    for sh in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ sh]
    s = lanes[..., 0]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def emulate32(c, order, grads="both"):
    """dict(ce, depth, loss, count, g_logp) of a float32 torch evaluation of case c in the order of the vec4 or the scalar
    kernels (torch's float32 exp and pow stand in for the device's)."""
    v, dc, m = c["logp"], c["dc"], c["mask"]
    B, D, H, W = v.shape
    from_depth = c["depth_gt"] is not None
    if from_depth:
        pw = torch.tensor(c["pow"], dtype=torch.float32)
        sig = torch.sqrt(torch.tensor(c["variance"], dtype=torch.float32))
        den = 2.0 * (sig * sig if float(pw) == 2.0 else torch.pow(sig, pw))
        z = c["depth_gt"]

        def gs(k):
            a = (dc[k] - z).abs()
            return torch.exp(-(a * a if float(pw) == 2.0 else torch.pow(a, pw)) / den)
        S = _sum_over_planes(gs, D, order)
        num = _sum_over_planes(lambda k: gs(k) * v[:, k], D, order)
        slp = _sum_over_planes(lambda k: v[:, k], D, order)
        ce = torch.where(S > 0, -(num / S), slp)
        lab = torch.stack([torch.where(S > 0, gs(k) / S, torch.full_like(S, -1.0)) for k in range(D)], 1)
    else:
        lab = c["label"]
        ce = -_sum_over_planes(lambda k: lab[:, k] * v[:, k], D, order)
    depth = _sum_over_planes(lambda k: dc[k] * torch.exp(v[:, k]), D, order)
    mm = torch.ones(B, H, W) if m is None else m
    w = torch.where(mm != 0, ce * mm, torch.zeros(()))
    tot = _workgroup_sums(w.view(B, -1), order).double().sum(1)
    count = torch.full((B,), float(H * W)) if m is None else (mm == 1).sum((1, 2)).float()
    loss = torch.where(count > 0, tot.float() / count, torch.zeros(()))
    out = {"ce": ce, "depth": depth, "loss": loss, "count": count}
    if grads:
        gl = c["g_loss"] if grads in ("both", "loss") else torch.zeros(B)
        n = count.view(B, 1, 1)
        coef = torch.where((n > 0) & (mm != 0), -(gl.view(B, 1, 1) * mm / n), torch.zeros(())).unsqueeze(1)
        o = torch.where(coef != 0, coef * lab, torch.zeros(()))
        if grads in ("both", "depth"):
            o = o + (c["g_depth"].unsqueeze(1) * dc.view(1, D, 1, 1)) * torch.exp(v)
        out["g_logp"] = o
    return out
