"""Shared by tests/test_fuse_host.py and tests/test_fuse_gpu.py: a float64 restatement of the DPV fusion (csrc/dpv_fuse.hip:
dpv_fuse_reg_kernel<64|128>, dpv_fuse_kernel) and of its gradient (csrc/dpv_fuse_bwd.hip), the classifier of columns, the
per-element a-priori bound a float32 evaluation is held to, a float32 emulation of the kernels' loops with the mistakes the bound
must catch, and the tables of shapes and column kinds.

The operation, per pixel, on float32 inputs x_k (log-DPV), dmap, mask, d_k, var, eps (models/models.py:666-672 with
utils/img_utils.py:31-47, :360-375):
    sigma = sqrt(var), two_var = 2 (sigma sigma)          in float32: that number is part of the operation's definition
    z_k = -(d_k - dmap)^2 / two_var,  v_k = exp(z_k),  S = sum_k v_k,  t_k = v_k / S,  NaN -> -1
    m_k = clamp(t_k mask + (1 / D)(1 - mask), eps, 1)
    u_k = exp(x_k + log m_k),  Su = sum_k u_k,  q_k = u_k / Su,  fused_k = clamp(q_k, eps, 1),  log fused_k
    c_k = pass_k (g_f,k q_k + g_l,k),  T = sum_k c_k,  g_x,k = c_k - q_k T        pass_k = (eps <= q_k <= 1)
forward64 evaluates everything after two_var in float64; grad64 takes pass_k as an argument.

Columns (classify).  normal: S64 >= 2^-100.  dead: every z_k < -110, so every float32 Gaussian is an exact 0 in every
implementation (exp(-110) = 2^-158.7 is below half the smallest denormal), S = 0, t = 0 / 0 = NaN -> -1 on every plane: the
restatement applies that rule (float64 alone would still divide there).  band: everything between -- a float32 S of a few
denormals, where 0 / 0 against 1e-45 / 1e-45 decides the result; no value is pinned there, the generators place no depth in
it (checked_depth raises) and every value test asserts that it holds no band column.

The bound (forward_bound, grad_bound) is a running error analysis: every quantity carries its float64 value X and a bound E_X
of the absolute error of the kernel's float32 X^, one line per operation of the kernel.  u = 2^-24 is the unit roundoff;
"flush(X)" is X where X < 2^-126 (1 + 1e-3) (a result below the normal range may be flushed to zero whole) and 2^-149
otherwise.  Constants: a correctly rounded operation u; the refined reciprocal 2 u (v_rcp_f32 is 1 ulp, the Newton step leaves
at most 1 ulp = 2 u); fuse_exp "about 1.5 ulp" = 3 u and fuse_log "about 2 ulp" = 4 u of the result plus 1e-7 absolute
(dpv_fuse_math.hpp).  libm's expf, logf (1 ulp) and the IEEE division (u) are inside the same constants, so the D > 128
kernels are held to the same formula.
    a  = |d_k - dmap|          E = u a
    s  = a a                   E = 3 u s
    z  = -s r(two_var)         E_z = 6 u |z|     (3 u from s, 2 u the reciprocal, u the product; |z| up to 110 on a normal column)
    v  = exp(z)                E_v = v (expm1(E_z) + 3 u exp(E_z)) + flush(v)
    S  = v_0 + ... + v_{D-1}   E_S = sum E_v + (D - 1) u S
    t  = v r(S)                E_t = (E_v + t E_S) / (S - E_S) + 3 u t + 2^-126      (0 on a dead column: t = -1 exactly)
    A  = t mask                E_A = |mask| E_t + u |A|
    B  = (1 / D)(1 - mask)     E_B = 3 u |B|      (the division, the difference, the product)
    m0 = A + B                 E_m0 = E_A + E_B + u |m0|
    m  = clamp(m0, eps, 1)     the interval [clamp(m0 - E_m0), clamp(m0 + E_m0)]
    L  = log m                 E_L = the larger log-ratio of m to the interval's ends + 4 u |L| + 1e-7
    y  = x + L                 E_y = E_L + u |y|      (|y| up to |x| + 36; x = -inf: u_k = 0 exactly)
    u_k = exp(y)               E_u = u_k (expm1(E_y) + 3 u exp(E_y)) + flush(u_k)
    Su = u_0 + ... + u_{D-1}   E_Su = sum E_u + (D - 1) u Su
    q  = u_k r(Su)             E_q = (E_u + q E_Su) / (Su - E_Su) + 3 u q + 2^-126
    fused = clamp(q, eps, 1)   the interval [clamp(q - E_q), clamp(q + E_q)]: E_f = the larger distance to an end
    log fused                  E_l = the larger log-ratio to the interval's ends + 4 u |log fused| + 1e-7
and for the gradient, with the same pass_k on both sides,
    p  = g_f q                 E_p = |g_f| E_q + u |p|
    g  = p + g_l               E_g = E_p + u |g|      (only with both gradients present)
    c  = pass g                E_c = pass E_g
    T  = c_0 + ... + c_{D-1}   E_T = sum E_c + (D - 1) u sum |c|
    w  = q T                   E_w = E_q |T| + (q + E_q) E_T + u |w|
    g_x = c - w                E = E_c + E_w + u |g_x| + 2^-126
The products of the remaining first-order terms are covered by the factor 1 + 1e-3 (the large ones -- expm1, the log-ratios,
the quotients -- are carried exactly above).  No number in it comes from the kernels' output.

pass_k (pass_for): from the float64 q wherever |q - eps| exceeds E_q; within that margin the float32 q may fall on either
side and pass_k is taken from the evaluation's own forward (fused_k > eps).  No pixel is excluded.

The float32 emulation below (emulate32) reaches 0.294 (fused), 0.236 (log fused) and 0.989 (gradient, g_l alone: g_l - q T is
one subtraction and u |g_x| all the bound has there) of the bound on the host; measured on an MI355X: tests/test_fuse_gpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

from pdepth_amd import synth

EPS = torch.finfo(float).eps   # 2^-52 (utils/img_utils.py:12), exact in float32
VAR = 0.3
U32 = 2.0 ** -24
TINY32 = 2.0 ** -126
DENORM32 = 2.0 ** -149
SECOND_ORDER = 1e-3
NORMAL_S = 2.0 ** -100
DEAD_Z = -110.0
LOG_ABS = 1e-7

# (B, D, H, W): D reaches every dispatch pair (forward reg<64>, reg<128>, libm; backward FULL, !FULL, general-fast,
# general-libm), HW every edge of the 256-pixel workgroup, B = 3 once per path
CASES = (
    (3, 1, 1, 1),
    (2, 2, 1, 255),
    (3, 63, 9, 37),
    (3, 64, 16, 16),
    (1, 64, 257, 1),
    (3, 65, 257, 1),
    (1, 128, 16, 16),
    (3, 129, 1, 255),
    (1, 200, 9, 37),
)
CASE_IDS = ["x".join(map(str, c)) for c in CASES]
MODES = ("g_f", "g_l", "both")
KINDS = ("peaked_agree", "peaked_disagree", "unmasked", "fractional_0.25", "fractional_0.5", "fractional_1m", "dead_masked_far",
         "dead_masked_neg", "dead_fractional", "on_candidate", "edge_normal", "some_minus_inf", "shifted_base", "shifted_p30",
         "shifted_m30")
DEAD_KINDS = ("dead_masked_far", "dead_masked_neg", "dead_fractional")
ROUNDS = 3   # how often the kinds are dealt over a case's first pixels

_CACHE = {}


def cached(key, make):
    """References are computed once and shared: treat what comes back as read-only."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def two_var32(var):
    """2 * torch.pow(sqrt(var), 2) in float32, as the reference and the kernels form it."""
    sigma = torch.sqrt(torch.tensor(var, dtype=torch.float32))
    return float(2 * (sigma * sigma))


def candidates(D):
    return torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0).astype(np.float32))


# ---- float64 restatement ---------------------------------------------------------------------------------------------------
def forward64(logp, dmaps, masks, dc, var=VAR, eps=EPS):
    """Every quantity of the module docstring in float64 [B,D,H,W] ([B,1,H,W] for the sums), from the float32 inputs."""
    x = logp.float().double()
    D = x.shape[1]
    d = dc.float().double().view(1, -1, 1, 1)
    mk = masks.float().double().reshape(x.shape[0], 1, x.shape[2], x.shape[3])
    a = (d - dmaps.float().double().unsqueeze(1)).abs()
    z = -(a * a) / two_var32(var)
    v = torch.exp(z)
    S = v.sum(1, keepdim=True)
    dead = z.amax(1, keepdim=True) < DEAD_Z
    normal = S >= NORMAL_S
    t = torch.where(dead.expand_as(v), torch.full_like(v, float("nan")), v / S)
    t = torch.where(t != t, torch.full_like(t, -1.0), t)
    m0 = t * mk + (1.0 / D) * (1.0 - mk)
    m = m0.clamp(eps, 1.0)
    y = x + torch.log(m)
    u = torch.exp(y)
    Su = u.sum(1, keepdim=True)
    q = u / Su
    fused = q.clamp(eps, 1.0)
    return {"x": x, "mask": mk, "z": z, "v": v, "S": S, "dead": dead, "normal": normal, "band": ~(dead | normal), "t": t, "m0": m0,
            "m": m, "y": y, "u": u, "Su": Su, "q": q, "fused": fused, "logf": torch.log(fused), "eps": eps}


def grad64(f, g_f, g_l, passk):
    """g_x,k = c_k - q_k T with c_k = pass_k (g_f,k q_k + g_l,k); an absent gradient is zero."""
    g = torch.zeros_like(f["q"])
    if g_f is not None:
        g = g + g_f.double() * f["q"]
    if g_l is not None:
        g = g + g_l.double()
    c = torch.where(passk, g, torch.zeros_like(g))
    return c - f["q"] * c.sum(1, keepdim=True)


def classify(dmaps, dc, var=VAR):
    """(normal, dead, band) [B,H,W] bool."""
    f = forward64(torch.zeros(dmaps.shape[0], dc.numel(), *dmaps.shape[1:]), dmaps, torch.ones_like(dmaps), dc, var)
    return f["normal"][:, 0], f["dead"][:, 0], f["band"][:, 0]


def checked_depth(value, dc, var=VAR):
    """float32 `value`, refused if a column of that depth is in the band."""
    v = torch.tensor([[[float(value)]]], dtype=torch.float32)
    if bool(classify(v, dc, var)[2].any()):
        raise ValueError("depth %r is in the band of these candidates" % (value,))
    return float(v)


# ---- the bound -------------------------------------------------------------------------------------------------------------
def _flush(x):
    return torch.where(x < TINY32 * (1 + 1e-3), x, torch.zeros_like(x)) + DENORM32


def _exp_err(val, e_arg):
    e = torch.where(val == 0, torch.zeros_like(val), val * (torch.expm1(e_arg) + 3 * U32 * torch.exp(e_arg)))
    return torch.where(e != e, torch.full_like(e, float("inf")), e) + _flush(val)


def _log_err(val, lo, hi):
    return torch.maximum(torch.log(hi / val), torch.log(val / lo)) + 4 * U32 * torch.log(val).abs() + LOG_ABS


def forward_bound(f):
    """dict(q, fused, logf): the absolute error bounds of the module docstring, float64 [B,D,H,W]; inf on band columns."""
    D = f["x"].shape[1]
    eps, mk = f["eps"], f["mask"]
    E_z = 6 * U32 * f["z"].abs()
    E_v = _exp_err(f["v"], E_z)
    E_S = E_v.sum(1, keepdim=True) + (D - 1) * U32 * f["S"]
    den = f["S"] - E_S
    E_t = (E_v + f["t"] * E_S) / den + 3 * U32 * f["t"] + TINY32
    E_t = torch.where(den > 0, E_t, torch.full_like(E_t, float("inf")))
    E_t = torch.where(f["dead"].expand_as(E_t), torch.zeros_like(E_t), E_t)
    E_t = torch.where(f["band"].expand_as(E_t), torch.full_like(E_t, float("inf")), E_t)
    A, Bq = f["t"] * mk, (1.0 / D) * (1.0 - mk)
    E_A = torch.where(mk == 0, torch.zeros_like(E_t), mk.abs() * E_t) + U32 * A.abs()
    E_m0 = E_A + 3 * U32 * Bq.abs() + U32 * f["m0"].abs()
    E_L = _log_err(f["m"], (f["m0"] - E_m0).clamp(eps, 1.0), (f["m0"] + E_m0).clamp(eps, 1.0))
    E_y = torch.where(torch.isinf(f["y"]), torch.zeros_like(E_L), E_L + U32 * f["y"].abs())
    E_u = _exp_err(f["u"], E_y)
    E_Su = E_u.sum(1, keepdim=True) + (D - 1) * U32 * f["Su"]
    den = f["Su"] - E_Su
    E_q = (E_u + f["q"] * E_Su) / den + 3 * U32 * f["q"] + TINY32
    E_q = torch.where(den > 0, E_q, torch.full_like(E_q, float("inf")))
    lo, hi = (f["q"] - E_q).clamp(eps, 1.0), (f["q"] + E_q).clamp(eps, 1.0)
    E_f = torch.maximum(hi - f["fused"], f["fused"] - lo)
    E_l = _log_err(f["fused"], lo, hi)
    k = 1 + SECOND_ORDER
    return {"q": k * E_q, "fused": k * E_f, "logf": k * E_l}


def grad_bound(f, E_q, g_f, g_l, passk):
    D = f["x"].shape[1]
    q = f["q"]
    g, E_g = torch.zeros_like(q), torch.zeros_like(q)
    if g_f is not None:
        g = g_f.double() * q
        E_g = g_f.double().abs() * E_q + U32 * g.abs()
    if g_l is not None:
        g = g + g_l.double()
        E_g = E_g + (U32 * g.abs() if g_f is not None else 0.0)
    c = torch.where(passk, g, torch.zeros_like(g))
    E_c = torch.where(passk, E_g, torch.zeros_like(g))
    T = c.sum(1, keepdim=True)
    E_T = E_c.sum(1, keepdim=True) + (D - 1) * U32 * c.abs().sum(1, keepdim=True)
    w = q * T
    E_w = E_q * T.abs() + (q + E_q) * E_T + U32 * w.abs()
    return (1 + SECOND_ORDER) * (E_c + E_w + U32 * (c - w).abs() + TINY32)


def pass_for(f, E_q, own_fused):
    """pass_k: the float64 decision where q is further from eps than E_q, the evaluation's own forward inside that margin."""
    q, eps = f["q"], f["eps"]
    return torch.where((q - eps).abs() > E_q, (q >= eps) & (q <= 1.0), own_fused.double() > eps)


def ratio(got, want64, bound):
    """err / bound per element, float64; inf where the result is not finite (or the bound is zero and the error is not)."""
    err = (got.double() - want64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(got.double()) & torch.isfinite(r), r, torch.full_like(r, float("inf")))


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _normalised(x):
    return F.log_softmax(x.double(), dim=0).float()


def case(idx):
    """dict(shape, dc, logp, dmaps, masks [B,H,W], g_f, g_l, kinds {name: [(b, y, x)]}): float32, seeded.  The base is a
    normalised log-DPV of 3 randn, depths uniform in [3, 42] (moved off the band where D is small enough to have one inside the
    candidates' range), binary masks; the kinds are dealt over the first ROUNDS * len(KINDS) pixels, starting at a kind that
    depends on the case so that the one-pixel cases do not all hold the same three."""
    def make():
        B, D, H, W = CASES[idx]
        g = torch.Generator().manual_seed(9100 + idx)
        dc = candidates(D)
        logp = F.log_softmax(3 * torch.randn(B, D, H, W, generator=g), dim=1)
        dmaps = 3 + 39 * torch.rand(B, H, W, generator=g)
        band = classify(dmaps, dc)[2]
        nearest = dc[(dc.view(-1, 1, 1, 1) - dmaps.unsqueeze(0)).abs().argmin(0)]
        dmaps = torch.where(band, nearest + 1.0, dmaps)
        masks = (torch.rand(B, H, W, generator=g) < 0.5).float()
        g_f, g_l = torch.randn(B, D, H, W, generator=g), torch.randn(B, D, H, W, generator=g)
        ref_col = torch.round(_normalised(3 * torch.randn(D, generator=g)) * 2.0 ** 16) * 2.0 ** -16   # (+-30 is then exact in float32)
        kinds = {k: [] for k in KINDS}
        dlo, dhi = float(dc.min()), float(dc.max())
        for n in range(min(B * H * W, ROUNDS * len(KINDS))):
            kind = KINDS[(n + 4 * idx) % len(KINDS)]
            b, y, x = n // (H * W), (n // W) % H, n % W
            kinds[kind].append((b, y, x))
            col, depth, mask = None, None, 1.0   # (None: the base value stays)
            if kind == "peaked_agree":
                P = (7 * n) % D
                col = 3 * torch.randn(D, generator=g)
                col[P] += 60.0
                col, depth = _normalised(col), float(dc[P])
            elif kind == "peaked_disagree":   # the peak P has a prior of eps, the measured plane J a DPV of exp(-80)
                P = (5 * n) % D
                J = int(((dc - dc[P]).abs() - 20.0).abs().argmin())
                col = -80.0 + 0.5 * torch.randn(D, generator=g)
                col[P] = 0.0
                depth = float(dc[J])
            elif kind == "unmasked":
                mask = 0.0
            elif kind.startswith("fractional"):   # (the base depth stays)
                mask = {"0.25": 0.25, "0.5": 0.5, "1m": 1.0 - 2.0 ** -24}[kind.split("_")[1]]
            elif kind in DEAD_KINDS:
                col, depth, mask = ref_col, (-50.0 if kind == "dead_masked_neg" else 1000.0), (0.5 if kind == "dead_fractional" else 1.0)
            elif kind == "on_candidate":
                depth = float(dc[(3 * n) % D])
            elif kind == "edge_normal":       # the nearest candidate 6.4 m away: S64 = exp(-68.3) = 2^-98.5
                depth = dhi + 6.4 if (n // len(KINDS)) % 2 == 0 else dlo - 6.4
            elif kind == "some_minus_inf":
                mask = None
                col = logp[b, :, y, x].clone()
                col[torch.randperm(D, generator=g)[:D // 3]] = float("-inf")
            else:
                col = ref_col + {"base": 0.0, "p30": 30.0, "m30": -30.0}[kind.split("_")[1]]
                depth = float(dc[D // 2]) + 0.3
            if col is not None:
                logp[b, :, y, x] = col
            if depth is not None:
                dmaps[b, y, x] = checked_depth(depth, dc)
            if mask is not None:
                masks[b, y, x] = mask
        return {"shape": CASES[idx], "dc": dc, "logp": logp, "dmaps": dmaps, "masks": masks, "g_f": g_f, "g_l": g_l, "kinds": kinds}
    return cached(("case", idx), make)


def reference(idx):
    """dict(f = forward64, E = forward_bound, held [B,1,H,W] = normal | dead, n_band), cached."""
    def make():
        c = case(idx)
        f = forward64(c["logp"], c["dmaps"], c["masks"], c["dc"])
        return {"f": f, "E": forward_bound(f), "held": f["normal"] | f["dead"], "n_band": int(f["band"].sum())}
    return cached(("ref", idx), make)


def grads_of(c, mode):
    return (c["g_f"] if mode != "g_l" else None), (c["g_l"] if mode != "g_f" else None)


# ---- the comparisons both tests make ---------------------------------------------------------------------------------------
def check_forward(idx, fused, logf):
    """(worst ratio of fused, worst ratio of log fused) over every plane of every normal and dead column of the case."""
    r = reference(idx)
    assert r["n_band"] == 0, "band columns: %d" % r["n_band"]
    held = r["held"].expand_as(r["f"]["q"])
    assert bool(held.all())
    return (float(ratio(fused.cpu(), r["f"]["fused"], r["E"]["fused"])[held].max()),
            float(ratio(logf.cpu(), r["f"]["logf"], r["E"]["logf"])[held].max()))


def check_backward(idx, mode, grad, own_fused):
    """Worst ratio of the gradient against the float64 closed form, pass_k by pass_for, over every element of the case."""
    c, r = case(idx), reference(idx)
    assert r["n_band"] == 0, "band columns: %d" % r["n_band"]
    g_f, g_l = grads_of(c, mode)
    passk = pass_for(r["f"], r["E"]["q"], own_fused.cpu())
    want = grad64(r["f"], g_f, g_l, passk)
    return float(ratio(grad.cpu(), want, grad_bound(r["f"], r["E"]["q"], g_f, g_l, passk)).max())


# ---- float32 emulation of the kernels' loops -------------------------------------------------------------------------------
MISTAKES = ("d_next", "var_for_two_var", "mask_swapped", "nan_to_zero", "pass_inverted", "T_of_g_f_only", "batch_stride")
# the case and the mode each mistake is shown on, and the output that shows it (nan_to_zero cannot show: test_fuse_host.py)
MISTAKE_CASE = {"d_next": (3, "both", "forward"), "var_for_two_var": (3, "both", "forward"), "mask_swapped": (3, "both", "forward"),
                "pass_inverted": (3, "g_l", "backward"), "T_of_g_f_only": (3, "both", "backward"),
                "batch_stride": (3, "both", "forward")}


def emulate32(logp, dmaps, masks, dc, g_f=None, g_l=None, var=VAR, eps=EPS, mistake=None):
    """(fused, log fused, g_x | None) in float32, one torch operation (one rounding) per operation of dpv_fuse_kernel and
    dpv_fuse_bwd_kernel<false>, the sums in the kernels' order; all pixels of a plane at once.  `mistake` plants one of
    MISTAKES."""
    B, D, H, W = logp.shape
    HW = H * W
    x = logp.float()
    if mistake == "batch_stride":   # item b's column read at b * HW instead of b * D * HW
        flat = x.reshape(-1)
        b, k, p = torch.arange(B).view(B, 1, 1), torch.arange(D).view(1, D, 1), torch.arange(HW).view(1, 1, HW)
        x = flat[(b * HW + k * HW + p).reshape(-1)].reshape(B, D, H, W)
    dc = dc.float()
    if mistake == "d_next":
        dc = torch.roll(dc, -1)
    mask = masks.float().reshape(B, H, W)
    inv_mask = 1.0 - mask
    if mistake == "mask_swapped":
        mask, inv_mask = inv_mask, mask
    sigma = torch.sqrt(torch.tensor(var, dtype=torch.float32))
    two_var = sigma * sigma if mistake == "var_for_two_var" else 2.0 * (sigma * sigma)
    uni = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32)
    eps32 = torch.tensor(eps, dtype=torch.float32)

    def gauss(k):
        a = (dc[k] - dmaps.float()).abs()
        return torch.exp(-(a * a) / two_var)

    sumg = torch.zeros(B, H, W)
    for k in range(D):
        sumg = sumg + gauss(k)

    def unnorm(k):
        t = gauss(k) / sumg
        t = torch.where(t != t, torch.full_like(t, 0.0 if mistake == "nan_to_zero" else -1.0), t)
        m = torch.minimum(torch.maximum(t * mask + uni * inv_mask, eps32), torch.ones(()))
        return torch.exp(x[:, k] + torch.log(m))

    sumf = torch.zeros(B, H, W)
    for k in range(D):
        sumf = sumf + unnorm(k)
    q = torch.stack([unnorm(k) / sumf for k in range(D)], dim=1)
    fused = torch.minimum(torch.maximum(q, eps32), torch.ones(()))
    logf = torch.log(fused)
    if g_f is None and g_l is None:
        return fused, logf, None
    passk = (q <= eps32) if mistake == "pass_inverted" else ((q >= eps32) & (q <= 1.0))
    g = g_f.float() * q if g_f is not None else None
    if g_l is not None:
        g = g + g_l.float() if g is not None else g_l.float()
    c = torch.where(passk, g, torch.zeros_like(g))
    cT = torch.where(passk, g_f.float() * q, torch.zeros_like(g)) if (mistake == "T_of_g_f_only" and g_f is not None) else c
    T = torch.zeros(B, H, W)
    for k in range(D):
        T = T + cT[:, k]
    return fused, logf, c - q * T.unsqueeze(1)


# ---- probes of the agreement between the forward and the backward ------------------------------------------------------------
LADDER_PIXELS = 512


def ladder(D):
    """dict(logp [1,D,2,256], dmaps, masks, dc) of near_clamp_ladder: mask 0 and D a power of two, so the prior 1 / D is exact;
    x_0 = (i - 256) 2^-26 on pixel i, the other planes at the float32 nearest log eps plus j 2^-18 (one float32 step there),
    j in -1 .. 1 by plane.  q_k / eps = exp(x_k - log eps - x_0) / (1 + about D eps) moves by 2^-26, a quarter of a float32 ulp,
    per pixel and by 2^-17 over the ladder, which contains the distance of log eps from its float32 neighbours (at most 2^-19)."""
    assert D & (D - 1) == 0
    i = torch.arange(LADDER_PIXELS, dtype=torch.float64)
    logp = torch.empty(1, D, 2, 256)
    near = torch.tensor(float(np.log(EPS)), dtype=torch.float32).double()
    for k in range(1, D):
        logp[0, k] = float(near + ((k % 3) - 1) * 2.0 ** -18)
    logp[0, 0] = ((i - 256) * 2.0 ** -26).float().view(2, 256)
    return {"logp": logp, "dmaps": torch.full((1, 2, 256), 20.0), "masks": torch.zeros(1, 2, 256), "dc": candidates(D)}


def one_hot_probes(fused):
    """(g_l of probe 1, g_l of probe 2, j1, j2 [B,1,H,W]): one-hot on the largest and on the second-largest plane of fused."""
    order = fused.argsort(dim=1, descending=True)
    j1, j2 = order[:, :1], order[:, 1:2] if fused.shape[1] > 1 else order[:, :1]
    return (torch.zeros_like(fused).scatter(1, j1, 1.0), torch.zeros_like(fused).scatter(1, j2, 1.0), j1, j2)


def q_disagreements(fused, gx1, gx2, eps=EPS):
    """(planes where fused_k != -g_x,k, planes compared): probe 1 answers every plane but its own, probe 2 the plane of probe 1
    (where probe 2's own plane passes: otherwise T = 0 and the probe says nothing)."""
    _, _, j1, j2 = one_hot_probes(fused)
    own1 = torch.zeros_like(fused, dtype=torch.bool).scatter(1, j1, True)
    live2 = (fused.gather(1, j2) > eps) & (j2 != j1)
    use2 = own1 & live2
    live1 = fused.gather(1, j1) > eps
    compared = (fused > eps) & ((~own1 & live1) | use2)
    minus_g = torch.where(use2, -gx2, -gx1)
    return int(((fused != minus_g) & compared).sum()), int(compared.sum())
