"""Shared by tests/test_dpv_backward_host.py and tests/test_dpv_backward_gpu.py: float64 references of the backward of the DPV
reductions (csrc/dpv_bwd.hip), the per-element a-priori bound a float32 evaluation of them is held to, float32 evaluations
of the same formula for the host test (torch autograd and a restatement of the kernel's two loops, with the mistakes the
bound must catch), and the tables of shapes and column kinds.

The operation: x = logits (+ addend) [B,D,H,W], logp = log_softmax(x, dim=1), p = exp(logp), depth = sum_k d_k p_k.  With the
incoming gradients g_logp, g_prob [B,D,H,W] and g_depth [B,H,W], any of them absent (= zero):
    t_k = g_prob_k + g_depth d_k,    G_k = g_logp_k + p_k t_k,    g_x_k = G_k - p_k sum_j G_j.
The kernel differentiates from a SAVED float32 logp.  The reference takes logp in float64 from the float32 logits, the kernel
test hands the kernel that logp rounded to float32: a wrong or noisy forward cannot loosen the backward's bound.

The bound (reduce_bound).  u = EPS32 = 2^-24 is the unit roundoff of float32, L_k = |logp_k| (0 where logp_k = -inf: expf(-inf)
is exactly 0 and 0 times a finite number is exactly 0), s_k = |g_depth d_k|.  The kernel computes, one rounding per operation
(the objects are built with -ffp-contract=off, so no product is fused into a sum):
    p^  = expf(logp32)       logp32 = logp (1 + e), |e| <= u, leaves exp(logp32) = p (1 + L e); expf is documented to 1 ulp <= 2 u
                             of its result: p^ = p (1 + th), |th| <= (2 + L) u
    s^  = g_depth * d_k      error <= u s_k
    t^  = g_prob + s^        error <= u (s_k + |t_k|)
    m^  = p^ * t^            error <= u ((4 + L_k) p_k |t_k| + p_k s_k)
    G^  = g_logp + m^        error <= u E_k,  E_k = |G_k| + (4 + L_k) p_k |t_k| + p_k s_k
    S^  = G^_0 + ... + G^_{D-1}, in this order: D - 1 roundings, each at most u times a partial sum <= sum_j |G_j|:
                             error <= u (sum_j E_j + (D - 1) sum_j |G_j|)
    q^  = p^ * S^            error <= u ((3 + L_k) p_k |S| + p_k (sum_j E_j + (D - 1) sum_j |G_j|))
    out = G^ - q^            error <= u |g_x_k| + the errors of G^ and q^,  |g_x_k| <= |G_k| + p_k |S|,  |S| <= sum_j |G_j|
which adds up, with |G_k| <= |g_logp_k| + p_k |t_k|, to
    u ( 2 |g_logp_k| + (6 + L_k) p_k |t_k| + p_k s_k + p_k sum_j ((D + 4 + L_k) |G_j| + (4 + L_j) p_j |t_j| + p_j s_j) )
to first order in u.  An absent gradient makes its operation exact (0 + x), never worse.  The terms of second order are products
of at most D + 16 + max L factors (1 + u): the first-order bound is multiplied by 1 + 1e-3, and reduce_bound asserts
(D + 16 + max L) u < 1e-3.  Where a result falls below the normal range of float32 (p = e^-100 is a normal case of a peaked
column) the relative model fails by at most TINY32 = 2^-126 absolute per operation, with or without flush to zero:
TINY32 (|t_k| + sum_j (|G_j| + |t_j|) + 2 D + 6) is added; it matters only where the gradient itself is below 1e-30.

The bound is per element: a column where every gradient is small has a small bound, whatever the rest of the tensor holds.

L enters only as the error of the logp that is differentiated from: u L for a logp rounded once.  torch's float32 autograd (the
host test's second witness) differentiates from its own float32 log_softmax, logp = (x - max) - log(sum_j exp(x_j - max)):
u |x - max| <= u L for the first difference, u L for the last, and for the logarithm of the sum u (2 + log D) from its terms
(expf and their rounded arguments, weighted by the softmax: at most the entropy), u (D - 1) from the additions and 2 u log D
from logf: u (2 L + D + 1 + 3 log D) in all (torch32_logp_error).  It is held to the same formula with that in L's place; with
L itself it needs up to 1.56 times the bound (randn30, g_prob alone: p ~ e^-150, the gradient is p_k t_k and the bound
(6 + L) u p |t|), which is its forward's noise and no error of the derivation.  The bound is tight, not generous: the
restatement, fed the rounded logp, reaches 0.96 of it where p_k is small and g_x_k ~ g_logp_k lies just above a power of two --
the two additions round by up to u |g_logp_k| each, and 2 u |g_logp_k| is all the bound has there.

dpv_expect's backward: g_dpv_k = g_depth d_k exp(dpv_k) for BV_log (one product, expf to 2 u, one product: 4 u |g64|, plus the
same second-order factor and 2 TINY32 (1 + s_k)); without BV_log it is the float32 product g_depth * d_k, bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

from pdepth_amd import synth

EPS32 = 2.0 ** -24     # the unit roundoff of float32 (half of torch.finfo(torch.float32).eps)
EPS64 = 2.0 ** -53
TINY32 = 2.0 ** -126   # the smallest normal float32
SECOND_ORDER = 1e-3

# (B, D, H, W): the smallest shapes that reach each forward kernel and each edge of the backward's grid (256 pixels per
# workgroup, one thread per pixel, blockIdx.y = item)
CASES = (
    (1, 1, 1, 1),       # smallest shape
    (1, 2, 1, 3),       # HW not a multiple of 4
    (2, 3, 4, 4),       # D < 4: plane groups without a plane
    (3, 31, 16, 16),    # HW = 256; B = 3
    (2, 32, 1, 257),    # one live thread in the second workgroup; W not a multiple of 4
    (2, 33, 8, 36),     # 16 planes per lane, ragged
    (1, 64, 16, 24),    # the model's shape
    (2, 65, 12, 20),    # 32 planes per lane
    (1, 128, 4, 68),    # D at the vec4 limit
    (2, 129, 4, 8),     # D > 128: the forward's scalar kernel
    (1, 200, 3, 5),     # D well past the limit
)
CASE_IDS = ["x".join(map(str, c)) for c in CASES]
KINDS = ("randn0.1", "randn3", "randn30", "peaked", "tie", "flat", "offset", "masked")
# (g_logp, g_prob, g_depth) present: the seven non-empty subsets
SUBSETS = tuple((bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(1, 8))
ALL3 = (True, True, True)
MISTAKES = ("d_next", "no_psum", "gd_neighbour", "no_gprob", "exp_logits")

_CACHE = {}


def cached(key, make):
    """References are computed once and shared: treat what comes back as read-only."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def kinds_for(D):
    """A tie needs two planes, and so does a mask that never covers a whole column."""
    return tuple(k for k in KINDS if D >= 2 or k not in ("tie", "masked"))


def candidates(idx, D):
    """float32 [D]: powerf(5, 40, D, 1) on the even cases, unsorted uniform in [0.5, 60] on the odd ones."""
    if idx % 2 == 0:
        return torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0).astype(np.float32))
    return (0.5 + 59.5 * torch.rand(D, generator=torch.Generator().manual_seed(7300 + idx), dtype=torch.float64)).float()


def case(idx):
    """dict(shape, dc [D], g_logp, g_prob [B,D,H,W], g_depth [B,H,W]): float32, seeded."""
    def make():
        B, D, H, W = CASES[idx]
        g = torch.Generator().manual_seed(7100 + idx)
        return {"shape": CASES[idx], "dc": candidates(idx, D), "g_logp": torch.randn(B, D, H, W, generator=g),
                "g_prob": torch.randn(B, D, H, W, generator=g), "g_depth": torch.randn(B, H, W, generator=g)}
    return cached(("case", idx), make)


def grads_of(c, subset):
    """(g_logp | None, g_prob | None, g_depth | None) of a case for a subset."""
    return tuple(c[k] if on else None for k, on in zip(("g_logp", "g_prob", "g_depth"), subset))


def logits(idx, kind):
    """float32 [B,D,H,W] logits of one column kind."""
    def make():
        B, D, H, W = CASES[idx]
        g = torch.Generator().manual_seed(7200 + 16 * idx + KINDS.index(kind))
        x = torch.randn(B, D, H, W, generator=g)
        pix = torch.arange(B * H * W).reshape(B, 1, H, W)
        if kind.startswith("randn"):
            return x * float(kind[5:])
        if kind == "peaked":   # +60 on one plane per pixel; pixels 0, 1, 2, ... take planes 0, D - 1, 1, D - 2, ...
            plane = torch.where(pix % 2 == 0, (pix // 2) % D, D - 1 - (pix // 2) % D)
            return x.scatter_add(1, plane, torch.full_like(plane, 60.0, dtype=torch.float32))
        if kind == "tie":      # two equal maxima, 5 above the rest
            a = pix % D
            b = (a + 1 + (pix // D) % (D - 1)) % D
            top = x.amax(1, keepdim=True) + 5.0
            return x.scatter(1, a, top).scatter(1, b, top)
        if kind == "flat":
            return torch.zeros(B, D, H, W) + x[:, :1]
        if kind == "offset":
            return 3 * x + 1e4
        assert kind == "masked"   # -inf on a random third of the planes (at least one), never on a whole column
        n = max(1, D // 3)
        order = torch.rand(B, D, H, W, generator=g).argsort(dim=1)
        return (3 * x).scatter(1, order[:, :n], float("-inf"))
    return cached(("logits", idx, kind), make)


# ---- float64 references ----------------------------------------------------------------------------------------------------
def logp64(x32, addend=None):
    x = x32.double() if addend is None else x32.double() + addend.double()
    return F.log_softmax(x, dim=1)


def _z(g, like):
    return torch.zeros_like(like, dtype=torch.float64) if g is None else g.double()


def _terms(lp64, dc, g_logp, g_prob, g_depth):
    """p, t, G, s in float64 (absent gradients are zero); dc is rounded to float32 first."""
    p = torch.exp(lp64)
    d = dc.float().double().view(1, -1, 1, 1)
    gd = _z(g_depth, lp64[:, 0]).unsqueeze(1)
    t = _z(g_prob, lp64) + gd * d
    return p, t, _z(g_logp, lp64) + p * t, (gd * d).abs()


def closed_form64(lp64, dc, g_logp=None, g_prob=None, g_depth=None):
    """g_x_k = G_k - p_k sum_j G_j in float64."""
    p, _, G, _ = _terms(lp64, dc, g_logp, g_prob, g_depth)
    return G - p * G.sum(1, keepdim=True)


def autograd(x32, dc, g_logp=None, g_prob=None, g_depth=None, addend=None, dtype=torch.float64):
    """torch autograd of log_softmax -> exp -> sum_k d_k p_k in `dtype` -> the gradient of the logits (= of the addend)."""
    x = x32.to(dtype).clone().requires_grad_(True)
    z = x if addend is None else x + addend.to(dtype)
    lp = F.log_softmax(z, dim=1)
    prob = torch.exp(lp)
    depth = (prob * dc.float().to(dtype).view(1, -1, 1, 1)).sum(1)
    loss = 0
    for out, g in ((lp, g_logp), (prob, g_prob), (depth, g_depth)):
        if g is not None:
            loss = loss + (out * g.to(dtype)).sum()
    loss.backward()
    return x.grad


def torch32_logp_error(L, D):
    """The absolute error, in units of u, of the logp torch's float32 log_softmax leaves: see the module docstring."""
    return 2 * L + D + 1 + 3 * float(np.log(D))


def reduce_bound(lp64, dc, g_logp=None, g_prob=None, g_depth=None, unit=EPS32, logp_error=None):
    """The per-element bound of the module docstring, float64 [B,D,H,W].  logp_error(L, D) -> the absolute error of the logp
    the evaluation differentiates from, in units of u (None: L, a logp rounded once)."""
    D = lp64.shape[1]
    p, t, G, s = _terms(lp64, dc, g_logp, g_prob, g_depth)
    L = torch.where(torch.isinf(lp64), torch.zeros_like(lp64), lp64.abs())
    Lmax = float(L[torch.isfinite(L)].max()) if bool(torch.isfinite(L).any()) else 0.0
    assert (D + 16 + Lmax) * EPS32 < SECOND_ORDER
    e = L if logp_error is None else torch.where(torch.isinf(lp64), torch.zeros_like(lp64), logp_error(L, D))
    pt, aG = p * t.abs(), G.abs()
    sumG = aG.sum(1, keepdim=True)
    col = ((D + 4) * aG + (4 + e) * pt + p * s).sum(1, keepdim=True)
    first = 2 * _z(g_logp, lp64).abs() + (6 + e) * pt + p * s + p * (col + e * sumG)
    absolute = TINY32 * (t.abs() + (aG + t.abs()).sum(1, keepdim=True) + 2 * D + 6)
    return unit * (1 + SECOND_ORDER) * first + (absolute if unit == EPS32 else 0.0)


def reference(idx, kind, subset):
    """dict(lp64, lp32 = lp64 rounded to float32, g64 = the closed form, bound), cached."""
    def make():
        c = case(idx)
        lp = cached(("lp64", idx, kind), lambda: logp64(logits(idx, kind)))
        gs = grads_of(c, subset)
        return {"lp64": lp, "lp32": lp.float(), "g64": closed_form64(lp, c["dc"], *gs), "bound": reduce_bound(lp, c["dc"], *gs)}
    return cached(("ref", idx, kind, subset), make)


def ratio(got, want64, bound):
    """err / bound per element, float64; inf where the result is not finite (or the bound is zero and the error is not)."""
    err = (got.double() - want64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(got.double()) & torch.isfinite(r), r, torch.full_like(r, float("inf")))


# ---- float32 evaluations for the host test ---------------------------------------------------------------------------------
def restatement32(lp32, dc, g_logp=None, g_prob=None, g_depth=None, mistake=None, x32=None):
    """The two loops of dpv_reduce_bwd_kernel in float32, in its order, one torch operation (one rounding) per operation of
    the kernel, all pixels of a plane at once.  `mistake` plants one of MISTAKES (x32: the logits, for 'exp_logits')."""
    B, D, H, W = lp32.shape
    z32 = lambda g, like: torch.zeros_like(like) if g is None else g.float()
    gl, gp, gd = z32(g_logp, lp32), z32(g_prob, lp32), z32(g_depth, lp32[:, 0])
    dc = dc.float()
    if mistake == "d_next":
        dc = torch.roll(dc, -1)
    if mistake == "gd_neighbour":
        gd = torch.roll(gd.reshape(B, H * W), -1, dims=1).reshape(B, H, W)
    if mistake == "no_gprob":
        gp = torch.zeros_like(gp)
    src = x32.float() if mistake == "exp_logits" else lp32

    def G_of(k):
        p = torch.exp(src[:, k])
        return p, gl[:, k] + p * (gp[:, k] + gd * dc[k])

    total = torch.zeros(B, H, W)
    for k in range(D):
        total = total + G_of(k)[1]
    out = torch.empty_like(lp32)
    for k in range(D):
        p, G = G_of(k)
        out[:, k] = G if mistake == "no_psum" else G - p * total
    return out


# ---- dpv_expect ------------------------------------------------------------------------------------------------------------
def expect_g64_and_bound(dpv32, dc, g_depth):
    """g_dpv_k = g_depth d_k exp(dpv_k) in float64 from the float32 inputs, and 4 u |g64| (+ second order, + underflow)."""
    gd, d = g_depth.double().unsqueeze(1), dc.float().double().view(1, -1, 1, 1)
    g64 = gd * d * torch.exp(dpv32.double())
    return g64, 4 * EPS32 * (1 + SECOND_ORDER) * g64.abs() + 2 * TINY32 * (1 + (gd * d).abs())


def expect_reference(idx):
    """The input of dpv_expect's backward for a case (the 'randn3' log-DPV rounded to float32) and, for BV_log: g64 and its
    bound; without: the float32 product.  Cached."""
    def make():
        c = case(idx)
        dpv = reference(idx, "randn3", ALL3)["lp32"]
        g64, bound = expect_g64_and_bound(dpv, c["dc"], c["g_depth"])
        plain = (c["g_depth"].unsqueeze(1) * c["dc"].view(1, -1, 1, 1)).expand_as(dpv).contiguous()
        return {"dpv": dpv, "g64": g64, "bound": bound, "plain32": plain}
    return cached(("expect", idx), make)


# ---- the mistakes the bound must catch -------------------------------------------------------------------------------------
# With g_logp present a one-hot column hides d, g_prob and g_depth on principle: there the gradient depends on them through
# p (1 - p) ~ e^-60 only, against roundings of u |g_logp|.  Without g_logp every term of the bound scales with p_k and the
# mistake shows on the planes beside the peak.  A planted mistake must leave the bound under one of the two.
PLANT_SUBSETS = (ALL3, (False, True, True))


def planted_kinds(D):
    """The kinds of a case on which a mistake can show at all.  'masked' with D = 2 leaves one live plane: g_x is
    (-g_logp_1, g_logp_1) there whatever d, g_prob and g_depth are."""
    return tuple(k for k in kinds_for(D) if not (k == "masked" and D - max(1, D // 3) < 2))


def planted_factor(idx, kind, mistake):
    """The largest err / bound of the restatement with `mistake` planted, over PLANT_SUBSETS."""
    c, x = case(idx), logits(idx, kind)
    worst = 0.0
    for sub in PLANT_SUBSETS:
        r = reference(idx, kind, sub)
        got = restatement32(r["lp32"], c["dc"], *grads_of(c, sub), mistake=mistake, x32=x)
        worst = max(worst, float(ratio(got, r["g64"], r["bound"]).max()))
    return worst


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------
NONFINITE_CASE = 5                        # (2, 33, 8, 36)
NONFINITE_PIXELS = ((0, 3, 17), (1, 6, 35))   # (b, y, x): a NaN logit on plane 7; an all -inf column


def nonfinite_logits():
    x = logits(NONFINITE_CASE, "randn3").clone()
    (b0, y0, x0), (b1, y1, x1) = NONFINITE_PIXELS
    x[b0, 7, y0, x0] = float("nan")
    x[b1, :, y1, x1] = float("-inf")
    return x
