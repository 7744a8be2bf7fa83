"""Shared by tests/test_dpv_forward_host.py and tests/test_dpv_forward_gpu.py: a float64 restatement of the FORWARD of the DPV
reductions (csrc/dpv.hip, csrc/dpv_reduce_body.hpp, csrc/dpv_moments.hip: dpv_reduce, dpv_reduce_ex, dpv_expect, dpv_moments), the
per-element a-priori bound a float32 evaluation of it is held to, a float32 emulation of the kernels' two summation orders for
the host test (with the mistakes the bound must catch), and the tables of shapes, column kinds and dispatch.

The operation, per pixel, on float32 inputs: x_k = logits_k, or logits_k + addend_k formed IN FLOAT32 (one rounding, as the
kernels form it and as models/models.py:694 forms it: that number is the operation's input); everything after it in float64:
    m = max_k x_k,  a_k = x_k - m,  S = sum_k exp(a_k),  ls = log S,  logp_k = a_k - ls  (= log_softmax(x)_k),  p_k = exp(logp_k)
    depth = sum_k d_k p_k,   var = sum_k (d_k - depth)^2 p_k,   quarter = logp[:, :, ::4, ::4] cut to H // 4, W // 4
dpv_expect and dpv_moments take a volume v as it is: z_k = exp(v_k) (BV_log) or z_k = v_k (any sign, any sum), then
    depth = sum_k d_k z_k,   var = sum_k (d_k - depth)^2 z_k.

The bound (forward_bound, tail_bound).  u = EPS32 = 2^-24 is the unit roundoff of float32.  Every object is built with
-ffp-contract=off, so each operation below rounds once; expf and logf are taken at their documented 1 ulp <= 2 u of the
result (as tests/util_dpv_backward.py takes expf).  Each line: the kernel's float32 X^ against the float64 X, absolute error E_X.
    m                          exact (a maximum rounds nothing)
    a_k  = x_k - m             E_a = u |a_k|                                  (x_k = -inf: a_k = -inf exactly, E_a = 0)
    e_k  = expf(a_k)           E_e = (2 u + E_a) e_k + TINY32                 (exp of an argument off by E_a: e_k E_a)
    S    = sum_k e_k           E_S = sum_k E_e + R(e)                         (R: the additions, below; 1 <= S <= D)
    ls   = logf(S)             E_ls = E_S / S + 2 u |ls|
    lp_k = a_k - ls            E_lp = E_a + E_ls + u |lp_k|                   -> logp, quarter
    p_k  = expf(lp_k)          E_p = (2 u + E_lp) p_k + TINY32                -> prob
    t_k  = d_k * p_k           E_t = |d_k| E_p + u |t_k| + TINY32
    dep  = sum_k t_k           E_dep = sum_k E_t + R(t)                       -> depth
    dd_k = d_k - dep           E_dd = E_dep + u |dd_k|
    q_k  = dd_k * dd_k         E_q = 2 |dd_k| E_dd + E_dd^2 + u (|dd_k| + E_dd)^2
    w_k  = q_k * p_k           E_w = E_q (p_k + E_p) + q_k E_p + u (q_k + E_q)(p_k + E_p) + TINY32
    var  = sum_k w_k           E_var = sum_k E_w + R(w)                       -> var
E_dd^2 is carried, not left to the second order: on the peak plane of a peaked column dd = 0 and p = 1, the kernel's dd is the
rounding error of dep and its square, (u d)^2 ~ 1e-12, is the whole error of a variance of 1e-24.
The sums, R(.): each rounded addition errs by at most u times its own result and by at most the smaller operand (a sum that
returns the larger operand is off by the smaller one): R = sum over the additions of min(u |partial sum|, |addend|), the
partial sums evaluated in float64 IN THE KERNEL'S ORDER --
    'lanes'     (wave layout, dpv_reduce_lanes / plane_sum<true>): s_g = the planes k = g + 4 i in ascending i, g = 0 .. 3, then
                (s0 + s1) + (s2 + s3) (group_sum: xor 16, xor 32 -- the same bits in all four lanes, addition commutes);
    'ascending' (one pixel per thread: dpv_reduce_scalar_kernel, dpv_reduce_ex_pixel<false>, dpv_expect_kernel<.,4|1>, both
                dpv_moments kernels): k = 0, 1, ..., D - 1.
The first addition of a chain is 0 + x, exact; a plane group without a plane adds an exact 0.  An operand of the cap is known
to its relative error only; that factor, the products of first-order terms and the float64 arithmetic of this file are inside
1 + SECOND_ORDER = 1 + 1e-3, under the premise forward_bound asserts: (D + 16 + 2 max(|a|, |lp|)) u < 1e-3 and E_S / S,
E_lp < 1e-3.  A result below the normal range (p = e^-100 on a peaked column) fails the relative model by at most TINY32 =
2^-126 per operation, flushed to zero or not: the TINY32 terms.  For dpv_expect and dpv_moments the chain starts at z (tail_bound):
E_z = 2 u z + TINY32 (BV_log: expf of an exact input) or 0 (linear).  No number here comes from a kernel's output.

Which order a call runs (order_of restates launch_dpv_reduce, launch_dpv_reduce_ex, launch_dpv_expect, launch_dpv_moments of
csrc/dpv.hip and csrc/dpv_moments.hip, and launch_reduce_lp of csrc/dpv_half.hip):
    dpv_reduce      lanes iff H W % 4 == 0, D <= 128 and logits / logp / depth on 16-byte boundaries
    dpv_reduce_ex   lanes iff W % 4 == 0, D <= 128, every tensor on a 16-byte boundary and not (in place with an addend);
                    in place = logp written over the logits: a call that asks for no logp is not in place
    dpv_expect      lanes iff H W % 4 == 0, D <= 128 and the volume and depth on 16-byte boundaries  (D > 128: <.,4>, else <.,1>)
    dpv_moments     ascending always (D <= 64: reg<64>, D <= 128: reg<128>, else the re-reading kernel)
    fp16 / bf16     lanes iff W % 4 == 0 and D <= 128 (an address alone moves it to plane_sum<true>: the same order)
The shape table (CASES; RPL = planes per lane 8 | 16 | 32 for D <= 32 | 64 | 128), kernel reached by reduce / reduce_ex / expect:
    1x1x1x1     scalar / pixel / <.,1>          HW = 1                       2x33x8x36   vec4<16> / ex_vec4<16> / vec4<16>   ragged last wave
    1x2x1x3     scalar / pixel / <.,1>          HW % 4 != 0                  1x64x16x24  vec4<16> x3                        the model's shape
    2x3x4x4     vec4<8> / ex_vec4<8> / vec4<8>  D < 4: groups without plane  2x65x12x20  vec4<32> x3
    3x31x16x16  vec4<8> x3                      HW = 256, B = 3              1x128x4x68  vec4<32> x3                        D at the limit
    2x32x1x257  scalar / pixel / <.,1>          HW % 4 != 0                  2x129x4x8   scalar / pixel / <.,4>             D > 128
    1x200x3x5   scalar / pixel / <.,1>                                      1x40x4x6    vec4<16> / PIXEL / vec4<16>        HW % 4 == 0, W % 4 != 0
    1x24x4x8 +4 bytes   scalar / pixel / <.,1>  only the address keeps it out of the wave layout
    1x16x4x8 in place + addend   (reduce_ex) pixel, the dispatch's explicit exception; without the addend ex_vec4<8>

Exact expectations (exact_failures): on a -inf plane of a live column a_k = -inf, expf gives 0, lp_k = -inf, p_k = 0; on a
one-hot column S = expf(0) = 1, logf(1) = 0, lp = 0, p = 1, depth = d_k * 1 + 0 + ... = d_k, dd = 0, var = 0: bit for bit.

Measured: the float32 emulation below, on the host, and the kernels on an MI355X -- tests/test_dpv_forward_host.py,
tests/test_dpv_forward_gpu.py."""
import torch
import torch.nn.functional as F

import util_dpv_backward as UB
from util_dpv_backward import EPS32, TINY32, SECOND_ORDER, cached  # noqa: F401

# (B, D, H, W), the logits 4 bytes off a 16-byte boundary, in place with an addend
CASES = tuple((s, False, False) for s in UB.CASES) + (
    ((1, 40, 4, 6), False, False),
    ((1, 24, 4, 8), True, False),
    ((1, 16, 4, 8), False, True),
)
SHAPES = tuple(c[0] for c in CASES)
CASE_IDS = ["x".join(map(str, s)) + ("-off4" if off else "") + ("-inplace-addend" if ipa else "") for s, off, ipa in CASES]
KINDS = UB.KINDS + ("offset_neg", "one_hot")
OUTPUTS = ("logp", "prob", "depth", "var", "quarter")
LANES, ASCENDING = "lanes", "ascending"
HALF_CASES = (3, 6, 7)   # 3x31x16x16, 1x64x16x24, 2x65x12x20: 8, 16 and 32 planes per lane


def kinds_for(D):
    """A tie needs two planes, and so does a mask that never covers a whole column."""
    return tuple(k for k in KINDS if D >= 2 or k not in ("tie", "masked"))


def order_of(op, shape, aligned=True, inplace_addend=False, half=False):
    """The summation order the dispatch gives a call: see the module docstring."""
    _, D, H, W = shape
    if op == "moments":
        return ASCENDING
    if half:
        return LANES if W % 4 == 0 and D <= 128 else ASCENDING
    quads = W % 4 == 0 if op == "reduce_ex" else (H * W) % 4 == 0
    assert op in ("reduce", "reduce_ex", "expect")
    return LANES if quads and D <= 128 and aligned and not (op == "reduce_ex" and inplace_addend) else ASCENDING


def candidates(idx):
    return UB.candidates(idx, SHAPES[idx][1])


def _generated(shape, kind, seed):
    """The recipe of util_dpv_backward.logits for a shape of this table."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, H, W, generator=g)
    pix = torch.arange(B * H * W).reshape(B, 1, H, W)
    if kind.startswith("randn"):
        return x * float(kind[5:])
    if kind == "peaked":
        plane = torch.where(pix % 2 == 0, (pix // 2) % D, D - 1 - (pix // 2) % D)
        return x.scatter_add(1, plane, torch.full_like(plane, 60.0, dtype=torch.float32))
    if kind == "tie":
        a = pix % D
        b = (a + 1 + (pix // D) % (D - 1)) % D
        top = x.amax(1, keepdim=True) + 5.0
        return x.scatter(1, a, top).scatter(1, b, top)
    if kind == "flat":
        return torch.zeros(B, D, H, W) + x[:, :1]
    if kind == "offset":
        return 3 * x + 1e4
    assert kind == "masked"
    n = max(1, D // 3)
    order = torch.rand(B, D, H, W, generator=g).argsort(dim=1)
    return (3 * x).scatter(1, order[:, :n], float("-inf"))


def logits(idx, kind):
    """float32 [B,D,H,W] logits of one column kind: util_dpv_backward's for its shapes and kinds; offset_neg = 3 x - 1e4 and
    one_hot (every plane -inf but one, which moves with the pixel) from the same x."""
    def make():
        B, D, H, W = SHAPES[idx]
        old = idx < len(UB.CASES)
        if kind in UB.KINDS:
            return UB.logits(idx, kind) if old else _generated(SHAPES[idx], kind, 7200 + 16 * idx + UB.KINDS.index(kind))
        x3 = logits(idx, "randn3")
        if kind == "offset_neg":
            return x3 - 1e4
        assert kind == "one_hot"
        pix = torch.arange(B * H * W).reshape(B, 1, H, W)
        plane = torch.where(pix % 2 == 0, (pix // 2) % D, D - 1 - (pix // 2) % D)
        return torch.full((B, D, H, W), float("-inf")).scatter(1, plane, x3.gather(1, plane))
    return cached(("fwd_logits", idx, kind), make)


def addend(idx):
    return cached(("fwd_addend", idx), lambda: torch.randn(SHAPES[idx], generator=torch.Generator().manual_seed(7400 + idx)))


def summed(idx, kind):
    """logits + addend in float32: the input of the operation when there is an addend."""
    return cached(("fwd_summed", idx, kind), lambda: logits(idx, kind) + addend(idx))


# ---- float64 restatement ---------------------------------------------------------------------------------------------------
def _d(dc):
    return dc.float().double().view(1, -1, 1, 1)


def tail64(z, dc):
    """(depth, var) [B,H,W] of z [B,D,H,W] float64."""
    d = _d(dc)
    depth = (d * z).sum(1)
    return depth, ((d - depth.unsqueeze(1)) ** 2 * z).sum(1)


def forward64(x32, dc):
    """Every quantity of the module docstring in float64 from the float32 x (the addend already in it) and candidates."""
    x = x32.float().double()
    m = x.amax(1, keepdim=True)
    a = x - m
    e = torch.exp(a)
    S = e.sum(1, keepdim=True)
    ls = torch.log(S)
    lp = a - ls
    p = torch.exp(lp)
    depth, var = tail64(p, dc)
    H, W = x.shape[2:]
    return {"x": x, "a": a, "e": e, "S": S, "ls": ls, "logp": lp, "prob": p, "depth": depth, "var": var,
            "quarter": lp[:, :, ::4, ::4][:, :, :H // 4, :W // 4], "dc": dc}


def volume64(v32, dc, bv_log):
    """dpv_expect / dpv_moments of a given float32 volume: dict(z, depth, var) in float64."""
    z = torch.exp(v32.float().double()) if bv_log else v32.float().double()
    depth, var = tail64(z, dc)
    return {"z": z, "depth": depth, "var": var, "dc": dc, "bv_log": bv_log}


# ---- the bound -------------------------------------------------------------------------------------------------------------
def _chain(t):
    """t [B,n,H,W] added in ascending planes from 0: (the sum [B,H,W], sum over the additions of min(u |partial|, |addend|))."""
    if t.shape[1] == 0:
        z = torch.zeros_like(t[:, :0].sum(1))
        return z, z
    part = t.cumsum(1)
    return part[:, -1], torch.minimum(EPS32 * part[:, 1:].abs(), t[:, 1:].abs()).sum(1)


def _add(a, b):
    s = a + b
    return s, torch.minimum(EPS32 * s.abs(), torch.minimum(a.abs(), b.abs()))


def running(t, order):
    """R(t) of the module docstring, [B,H,W]."""
    if order == ASCENDING:
        return _chain(t)[1]
    assert order == LANES
    (s0, r0), (s1, r1), (s2, r2), (s3, r3) = (_chain(t[:, g::4]) for g in range(4))
    s01, r01 = _add(s0, s1)
    s23, r23 = _add(s2, s3)
    return r0 + r1 + r2 + r3 + r01 + r23 + _add(s01, s23)[1]


def _finite_abs(v):
    return torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v))


def tail_bound(z, E_z, dc, order):
    """(E_depth, E_var) [B,H,W] for depth = sum d z, var = sum (d - depth)^2 z with z known to E_z: without the second-order
    factor, which the callers apply."""
    d = _d(dc)
    u = EPS32
    t = d * z
    E_t = d.abs() * E_z + u * t.abs() + TINY32
    E_dep = E_t.sum(1) + running(t, order)
    dd = (d - t.sum(1, keepdim=True)).abs()
    E_dd = E_dep.unsqueeze(1) + u * dd
    q = dd * dd
    E_q = 2 * dd * E_dd + E_dd * E_dd + u * (dd + E_dd) ** 2
    za = z.abs()
    E_w = E_q * (za + E_z) + q * E_z + u * (q + E_q) * (za + E_z) + TINY32
    return E_dep, E_w.sum(1) + running(q * z, order)


def forward_bound(f, order):
    """dict(logp, prob [B,D,H,W], depth, var [B,H,W], quarter): the bounds of the module docstring on the live columns of
    f = forward64(...); a non-finite column (and a -inf plane's logp) is compared by pattern, not by these numbers."""
    u = EPS32
    D = f["x"].shape[1]
    aa, al = _finite_abs(f["a"]), _finite_abs(f["logp"])
    live = torch.isfinite(f["S"])
    big = float(torch.maximum(aa, al)[live.expand_as(aa)].max()) if bool(live.any()) else 0.0
    assert (D + 16 + 2 * big) * u < SECOND_ORDER
    clean = lambda v: torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    e, p, S = clean(f["e"]), clean(f["prob"]), torch.where(live, f["S"], torch.ones_like(f["S"]))
    E_a = u * aa
    E_e = (2 * u + E_a) * e + TINY32
    E_S = E_e.sum(1, keepdim=True) + running(e, order).unsqueeze(1)
    E_ls = E_S / S + 2 * u * clean(f["ls"]).abs()
    E_lp = E_a + E_ls + u * al
    assert float((E_S / S).max()) < SECOND_ORDER and float(E_lp.max()) < SECOND_ORDER
    E_p = (2 * u + E_lp) * p + TINY32
    E_dep, E_var = tail_bound(p, E_p, f["dc"], order)
    k = 1 + SECOND_ORDER
    H, W = f["x"].shape[2:]
    return {"logp": k * E_lp, "prob": k * E_p, "depth": k * E_dep, "var": k * E_var,
            "quarter": k * E_lp[:, :, ::4, ::4][:, :, :H // 4, :W // 4]}


def volume_bound(v, order):
    """dict(depth, var) for v = volume64(...)."""
    z = torch.where(torch.isfinite(v["z"]), v["z"], torch.zeros_like(v["z"]))
    E_z = 2 * EPS32 * z + TINY32 if v["bv_log"] else torch.zeros_like(z)
    E_dep, E_var = tail_bound(z, E_z, v["dc"], order)
    return {"depth": (1 + SECOND_ORDER) * E_dep, "var": (1 + SECOND_ORDER) * E_var}


def half_rounding(p64, E_p, dtype):
    """E_p plus the one rounding of prob to fp16 / bf16: half an ulp of the rounded value, or of the type's subnormal step."""
    uh, step = {torch.float16: (2.0 ** -11, 2.0 ** -25), torch.bfloat16: (2.0 ** -8, 2.0 ** -134)}[dtype]
    return E_p + uh * (p64.abs() + E_p) + step


def ratio(got, want64, bound):
    """err / bound per element, float64.  Where the reference is not finite the result must be the same non-finite value
    (NaN for NaN): 0 if it is, inf if not; inf where a finite reference meets a non-finite result or a zero bound an error."""
    got = got.detach().cpu().double()
    assert got.shape == want64.shape, (got.shape, want64.shape)
    err = (got - want64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got) & torch.isfinite(r), r, torch.full_like(r, float("inf")))
    same = (got == want64) | (got.isnan() & want64.isnan())
    pattern = torch.where(same, torch.zeros_like(r), torch.full_like(r, float("inf")))
    return torch.where(torch.isfinite(want64), r, pattern)


def worst(got, want64, bound):
    r = ratio(got, want64, bound)
    return float(r.max()) if r.numel() else 0.0


# ---- references, cached ----------------------------------------------------------------------------------------------------
def reference(idx, kind, with_addend=False):
    """dict(x32, f = forward64): of logits(idx, kind), or of logits + addend formed in float32."""
    def make():
        x = summed(idx, kind) if with_addend else logits(idx, kind)
        return {"x32": x, "f": forward64(x, candidates(idx))}
    return cached(("fwd_ref", idx, kind, with_addend), make)


def bound(idx, kind, with_addend, order):
    return cached(("fwd_bound", idx, kind, with_addend, order), lambda: forward_bound(reference(idx, kind, with_addend)["f"], order))


def volume(idx, kind, bv_log):
    """The float32 volume dpv_expect and dpv_moments are given.  BV_log: the float64 log-softmax rounded to float32 (-inf planes
    stay).  Linear: the logits themselves -- neither normalised nor non-negative -- or, where they hold -inf, the float64
    softmax rounded to float32."""
    def make():
        f = reference(idx, kind)["f"]
        if bv_log:
            return f["logp"].float()
        return f["prob"].float() if kind in ("masked", "one_hot") else logits(idx, kind)
    return cached(("fwd_volume", idx, kind, bv_log), make)


def volume_reference(idx, kind, bv_log):
    return cached(("fwd_vref", idx, kind, bv_log), lambda: volume64(volume(idx, kind, bv_log), candidates(idx), bv_log))


def check_outputs(out, f, E):
    """{name: worst err / bound} over the outputs present in `out` (a dict as ops.dpv_reduce_ex returns it)."""
    return {k: worst(out[k], f[k], E[k]) for k in OUTPUTS if k in out and out[k] is not None}


def exact_failures(x32, dc, out):
    """How many elements break the exact expectations of the module docstring, over the outputs present in `out`."""
    x = x32.float()
    live = torch.isfinite(x.amax(1, keepdim=True)) & ~x.isnan().any(1, keepdim=True)
    minus = (x == float("-inf")) & live
    hot = live[:, 0] & ((x > float("-inf")).sum(1) == 1)
    peak = (x > float("-inf")) & hot.unsqueeze(1)
    get = lambda k: out[k].detach().cpu().float() if out.get(k) is not None else None
    bad = 0
    lp, p, dep, var = get("logp"), get("prob"), get("depth"), get("var")
    if lp is not None:
        bad += int((lp[minus] != float("-inf")).sum()) + int((lp[peak] != 0).sum())
    if p is not None:
        bad += int((p[minus] != 0).sum()) + int((p[peak] != 1).sum())
    if dep is not None:
        dk = (torch.where(peak, dc.float().view(1, -1, 1, 1).expand_as(x), torch.zeros_like(x))).sum(1)
        bad += int((dep[hot] != dk[hot]).sum())
    if var is not None:
        bad += int((var[hot] != 0).sum())
    return bad


# ---- float32 emulation of the kernels' orders, for the host test -------------------------------------------------------------
MISTAKES = ("lp_fused", "group_max", "tail_dropped", "d_next", "var_raw", "fill_zero")
# the case, the kind, the order and the output each mistake is shown on
MISTAKE_CASE = {
    "lp_fused": (6, "offset", LANES, "logp"),         # x - (m + ls): the sum rounds at ulp(1e4)
    "group_max": (6, "randn3", LANES, "logp"),        # each plane group subtracts its own maximum, the sums combined as one
    "tail_dropped": (5, "flat", LANES, "logp"),       # D = 33: plane 32 left out of the sum of exponentials
    "d_next": (6, "randn3", LANES, "depth"),          # d_{k+1} in the expectation
    # E[d^2] - E[d]^2: cancellation at u d^2 where the variance is small.  (Not 'peaked': there p^ = 1 and d * 1 are exact, both
    # forms give the same bits on the peak plane, and the neighbours' e^-60 is below either form's reach.)
    "var_raw": (6, "randn30", LANES, "var"),
    "fill_zero": (5, "offset_neg", LANES, "logp"),    # D = 33: the absent planes of a lane enter the maximum as 0
}


def _sum32(D, order, term):
    """sum_k term(k) in float32 in the kernel's order; term(k) -> [B,H,W] float32, or None for a plane left out."""
    def chain(ks):
        s = None
        for k in ks:
            t = term(k)
            if t is not None:
                s = t if s is None else s + t   # (0 + t is exact)
        return s
    if order == ASCENDING:
        return chain(range(D))
    s = [chain(range(g, D, 4)) for g in range(4)]
    pair = lambda a, b: b if a is None else (a if b is None else a + b)
    return pair(pair(s[0], s[1]), pair(s[2], s[3]))


def emulate_tail32(z, dc, order, mistake=None):
    """(depth, var) in float32 from z [B,D,H,W] float32: the kernels' operations in their order."""
    D = z.shape[1]
    dc = dc.float()
    de = torch.roll(dc, -1) if mistake == "d_next" else dc
    depth = _sum32(D, order, lambda k: de[k] * z[:, k])
    if mistake == "var_raw":
        return depth, _sum32(D, order, lambda k: (dc[k] * dc[k]) * z[:, k]) - depth * depth

    def w(k):
        dd = dc[k] - depth
        return (dd * dd) * z[:, k]
    return depth, _sum32(D, order, w)


def emulate32(x32, dc, order, mistake=None):
    """dict(logp, prob, depth, var, quarter) in float32, one torch operation (one rounding) per operation of dpv_reduce_lanes
    (order 'lanes') or of the one-pixel-per-thread kernels ('ascending'); `mistake` plants one of MISTAKES."""
    x = x32.float()
    B, D, H, W = x.shape
    rpl = 8 if D <= 32 else 16 if D <= 64 else 32
    m = x.amax(1)
    if mistake == "fill_zero" and D < 4 * rpl:
        m = torch.maximum(m, torch.zeros(()))
    if mistake == "group_max":
        mg = [x[:, g::4].amax(1) if g < D else None for g in range(4)]
        a = torch.stack([x[:, k] - mg[k % 4] for k in range(D)], 1)
    else:
        a = x - m.unsqueeze(1)
    last = 4 * (D // 4) if mistake == "tail_dropped" else D
    S = _sum32(D, order, lambda k: torch.exp(a[:, k]) if k < last else None)
    ls = torch.log(S)
    lp = x - (m + ls).unsqueeze(1) if mistake == "lp_fused" else a - ls.unsqueeze(1)
    p = torch.exp(lp)
    depth, var = emulate_tail32(p, dc, order, mistake)
    return {"logp": lp, "prob": p, "depth": depth, "var": var, "quarter": lp[:, :, ::4, ::4][:, :, :H // 4, :W // 4]}


def emulate_volume32(v32, dc, bv_log, order):
    z = torch.exp(v32.float()) if bv_log else v32.float()
    depth, var = emulate_tail32(z, dc, order)
    return {"depth": depth, "var": var}


# ---- non-finite columns ----------------------------------------------------------------------------------------------------
NONFINITE_CASES = (5, 4)   # 2x33x8x36: wave layout, the second workgroup's last wave has 8 of 16 quads; 2x32x1x257: one pixel per thread
PLANTS = ("nan_plane", "inf_plane", "minus_inf_column")


def nonfinite_pixels(shape):
    """[(b, pixel)]: pixel 0, the last pixel, one pixel in each position of a quad, one in the last (ragged) wave."""
    B, _, H, W = shape
    HW = H * W
    last_wave = 64 * ((HW - 1) // 64)
    want = [0, HW - 1, 4 * 5 + 1, 4 * 9 + 2, 4 * 12 + 3, 4 * 14, last_wave + 9]
    pix = sorted({p for p in want if 0 <= p < HW})
    return [(i % B, p) for i, p in enumerate(pix)]


def plant(x32, shape, what):
    """(a copy of x32 with `what` planted in nonfinite_pixels, the mask [B,H,W] of those pixels)."""
    B, D, H, W = shape
    x = x32.clone().reshape(B, D, H * W)
    mask = torch.zeros(B, H * W, dtype=torch.bool)
    for n, (b, p) in enumerate(nonfinite_pixels(shape)):
        k = (3 * n + 1) % D
        if what == "nan_plane":
            x[b, k, p] = float("nan")
        elif what == "inf_plane":
            x[b, k, p] = float("inf")
        else:
            x[b, :, p] = float("-inf")
        mask[b, p] = True
    return x.reshape(B, D, H, W), mask.reshape(B, H, W)
