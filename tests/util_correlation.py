"""Shared by tests/test_correlation_host.py and tests/test_correlation_gpu.py: a float64 restatement of the correlation
operator (include/pdepth.h; csrc/correlation.hip: correlation_fwd_kernel<R>, correlation_fwd_mfma_kernel<KMAX>,
correlation_bwd_kernel<WANT1,WANT2>; csrc/correlation_general.hip: corr_general_fwd, corr_general_bwd), forward and both
gradients, the a-priori per-element bound a float32 (or fp16 I/O) evaluation of it is held to, a restatement of the dispatch
(which_kernel), float32 emulations of the kernels' summation orders and the mistakes the bound must catch for the host test,
and the input families.

The operation, on float32 or fp16 inputs widened exactly, with kr = (k - 1) / 2, dr = md / s2, ds = 2 dr + 1, n = k k C, in the
coordinates of the inputs zero-padded by `pad` on every side (in1p, in2p), (y1, x1) = (oy, ox) s1 + md:
    out[b, (tj+dr) ds + (ti+dr), oy, ox] = 1/n sum_{j,i in [-kr,kr]} sum_c in1p[b,c,y1+j,x1+i] in2p[b,c,y1+tj s2+j, x1+ti s2+i]
    d in1p[b,c,y1+j,x1+i]             += 1/n go[b,tc,oy,ox] in2p[b,c,y1+tj s2+j, x1+ti s2+i]      over (tj,ti,j,i) and (oy,ox)
    d in2p[b,c,y1+tj s2+j,x1+ti s2+i] += 1/n go[b,tc,oy,ox] in1p[b,c,y1+j,x1+i]
the gradients being the padded ones cut back to the image: per input element the gather sums at the top of
correlation_general.hip.  For a fixed (tj,ti,j,i) the outputs map one to one to the padded elements they pair, so adding the
whole plane of terms of one (tj,ti,j,i) at a time gives every element exactly its gather sum, at most m = ds ds k k terms.
Everything is evaluated ON the zero-padded arrays and no term is skipped, so 0 * inf = NaN falls out of the arithmetic: an inf or
NaN paired with padding gives NaN, as in the reference's padded buffers (correlation_cuda_kernel.cu:88-96).  Only terms whose
output (oy, ox) does not exist are absent.  Next to every sum S the reference returns A: the same sum with every product
replaced by its absolute value, times 1/n.

The bound.  u = 2^-24, gamma_m = m u / (1 - m u).  A sum of m products by m fused multiply-adds, in any order and however it is
split into chains that are added afterwards, is off by at most gamma_m sum |products| (each product enters the result through
at most m roundings, one per addition above it); the rounding of 1/n to float32 and of the final product add two more factors:
    forward,  fp32:  |got - ref| <= gamma_(n+2) A + (n + 2) 2^-126,      n = k k C
    backward, fp32:  the same with m = ds ds k k for n and A built from |go * other|
    fp16 I/O      :  E32 + 2^-11 (|ref| + E32) + 2^-25                  (one rounding of the output, normal or subnormal)
2^-126 per operation covers a flushed or rounded subnormal (TINY32 of tests/util_dpv_forward.py).  Every output element is
compared.  Where the reference is not finite, the result must be of the same class (+inf, -inf, NaN): ratio().  No number here
comes from a kernel's output.

Which kernel a call runs (which_kernel restates the dispatch of csrc/correlation.hip: corr_fast_path, the two LDS predicates and
launch_correlation_forward):
    fp16, or not (k = 1, s1 = 1, pad = md >= 1, md % s2 = 0, md / s2 <= 4)                                 general
    forward : LDS (8 * 16 * (16 + 2 md) + 8 * 256) * 4 > 160 KiB   (md >= 145)                             general
              C <= 256, md <= 16, C H W 4 < 2^31, B H ceil(W / 64) < 2^31       matrix pipe, KMAX 16 | 32 | 64 for C <= 64 | 128 | 256
              otherwise                                             scalar<R>, R = md / s2; its LDS opts in above 64 KiB (md >= 49)
    backward: LDS 2 * 8 * (16 + 2 md)^2 * 4 > 160 KiB              (md >= 18)                              general
              otherwise                                             fast backward, with opt-in LDS above 64 KiB (md >= 9)
"""
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
LDS_OPT_IN, LDS_CAP = 64 * 1024, 160 * 1024

GENERAL, FAST_BWD, FAST_BWD_OPT_IN = "general", "fast backward", "fast backward, opt-in LDS"
MFMA = {16: "matrix pipe<16>", 32: "matrix pipe<32>", 64: "matrix pipe<64>"}
SCALAR = {r: "scalar<%d>" % r for r in (1, 2, 3, 4)}

# ---- geometry and dispatch -------------------------------------------------------------------------------------------------
def geometry(H, W, cfg):
    """(kr, dr, ds, oH, oW) of cfg = (pad, k, md, s1, s2); asserts what the C entries require of a configuration."""
    pad, k, md, s1, s2 = cfg
    kr, dr = (k - 1) // 2, md // s2
    assert pad >= 0 and k >= 1 and k % 2 == 1 and md >= 0 and s1 >= 1 and s2 >= 1 and md - dr * s2 - kr >= 0, cfg
    ph, pw = H + 2 * pad - 2 * (kr + md), W + 2 * pad - 2 * (kr + md)
    assert ph > 0 and pw > 0, (H, W, cfg)
    return kr, dr, 2 * dr + 1, -(-ph // s1), -(-pw // s1)


def fast_path(cfg):
    pad, k, md, s1, s2 = cfg
    return k == 1 and s1 == 1 and pad == md and md >= 1 and md % s2 == 0 and md // s2 <= 4


def forward_lds(md):
    return (8 * 16 * (16 + 2 * md) + 8 * 256) * 4


def backward_lds(md):
    return 2 * 8 * (16 + 2 * md) ** 2 * 4


def which_kernel(shape, cfg, half=False, backward=False):
    """The kernel that serves a call on [B,C,H,W] inputs: see the module docstring."""
    B, C, H, W = shape
    md, s2 = cfg[2], cfg[4]
    if half or not fast_path(cfg):
        return GENERAL
    if backward:
        lds = backward_lds(md)
        return GENERAL if lds > LDS_CAP else FAST_BWD_OPT_IN if lds > LDS_OPT_IN else FAST_BWD
    if forward_lds(md) > LDS_CAP:
        return GENERAL
    if C <= 256 and md <= 16 and C * H * W * 4 < 2 ** 31 and B * H * ((W + 63) // 64) < 2 ** 31:
        return MFMA[16 if C <= 64 else 32 if C <= 128 else 64]
    return SCALAR[md // s2]


# ---- float64 restatement ---------------------------------------------------------------------------------------------------
MUTANTS = ("drop_channel", "swap_dy_dx", "flip_sign", "off_by_one", "inv_c_plus_1", "unmirrored_g2", "clamped_border")
EXTRA = 1   # one more ring of padding than `pad`, never read by the operation: room for the off-by-one mutant


def reference(x1, x2, go, cfg, mutant=None):
    """dict(out, A_out[, g1, A_g1, g2, A_g2]) in float64 from float32 / fp16 host tensors; `mutant` plants one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    pad, k, md, s1, s2 = cfg
    B, C, H, W = x1.shape
    kr, dr, ds, oH, oW = geometry(H, W, cfg)
    P = pad + EXTRA
    mode = "replicate" if mutant == "clamped_border" else "constant"
    a = F.pad(x1.float().double(), [P] * 4, mode=mode)
    b = F.pad(x2.float().double(), [P] * 4, mode=mode)
    if mutant == "drop_channel":
        a = a.clone()
        a[:, C - 1] = 0
    inv_n = 1.0 / (k * k * (C + 1 if mutant == "inv_c_plus_1" else C))
    ys = (md + EXTRA + s1 * torch.arange(oH))[:, None]
    xs = (md + EXTRA + s1 * torch.arange(oW))[None, :]
    out = torch.zeros(B, ds * ds, oH, oW, dtype=torch.float64)
    A_out = torch.zeros_like(out)
    want_g = go is not None
    if want_g:
        g = go.float().double()
        assert g.shape == out.shape, (g.shape, out.shape)
        g1, A1, g2, A2 = (torch.zeros_like(a) for _ in range(4))
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            tc = (tj + dr) * ds + (ti + dr)
            if mutant == "swap_dy_dx":
                tc = (ti + dr) * ds + (tj + dr)
            oy2, ox2 = tj * s2, ti * s2
            if mutant == "flip_sign":
                oy2, ox2 = -oy2, -ox2
            if mutant == "off_by_one" and (tj, ti) == (dr, 0):
                ox2 += 1
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    i1 = (ys + j, xs + i)
                    i2 = (ys + oy2 + j, xs + ox2 + i)
                    p1, p2 = a[:, :, i1[0], i1[1]], b[:, :, i2[0], i2[1]]
                    prod = p1 * p2
                    out[:, tc] += prod.sum(1)
                    A_out[:, tc] += prod.abs().sum(1)
                    if want_g:
                        gt = g[:, tc:tc + 1]
                        t1, t2 = gt * p2, gt * p1
                        if mutant == "unmirrored_g2":   # the term lands on, and is read at, the pixel mirrored the wrong way
                            i2 = (ys - oy2 + j, xs - ox2 + i)
                            t2 = gt * a[:, :, i2[0], i2[1]]
                        g1[:, :, i1[0], i1[1]] += t1
                        A1[:, :, i1[0], i1[1]] += t1.abs()
                        g2[:, :, i2[0], i2[1]] += t2
                        A2[:, :, i2[0], i2[1]] += t2.abs()
    r = {"out": out * inv_n, "A_out": A_out * inv_n}
    if want_g:
        cut = lambda t: t[:, :, P:P + H, P:P + W] * inv_n
        r.update(g1=cut(g1), A_g1=cut(A1), g2=cut(g2), A_g2=cut(A2))
    return r


# ---- the bound -------------------------------------------------------------------------------------------------------------
def gamma(m):
    assert m * EPS32 < 0.01
    return m * EPS32 / (1 - m * EPS32)


def terms(C, H, W, cfg, backward):
    """The number of products behind one element: n = k k C forward, m = ds ds k k backward."""
    kr, dr, ds, _, _ = geometry(H, W, cfg)
    k = cfg[1]
    return ds * ds * k * k if backward else k * k * C


def bound(ref, A, m, half=False):
    """The module docstring's bound per element (float64); NaN / inf where A is (the class is compared there)."""
    e = gamma(m + 2) * A + (m + 2) * TINY32
    return e + 2.0 ** -11 * (ref.abs() + e) + 2.0 ** -25 if half else e


def classes(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    t = t.double()
    return (t == float("inf")) * 1 + (t == float("-inf")) * 2 + t.isnan() * 3


def ratio(got, ref, E):
    """err / bound per element, float64: inf where the classes differ, 0 where both are the same non-finite class."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    same = classes(got) == classes(ref)
    fin = torch.isfinite(ref) & torch.isfinite(got)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / E)
    r = torch.where(fin, r, torch.zeros_like(r))
    return torch.where(same & ~r.isnan(), r, torch.full_like(r, float("inf")))


def worst(got, ref, E):
    r = ratio(got, ref, E)
    return float(r.max()) if r.numel() else 0.0


def check(got, r, name, shape, cfg, half=False):
    """worst err / bound of one result (name: out | g1 | g2) against reference() r."""
    _, C, H, W = shape
    m = terms(C, H, W, cfg, name != "out")
    return worst(got, r[name], bound(r[name], r["A_" + name], m, half))


# ---- input families --------------------------------------------------------------------------------------------------------
FAMILIES = ("randn", "offset", "alternating", "tiny", "huge")
HALF_FAMILIES = ("randn", "offset", "alternating")   # 1e-15 and 1e+15 are outside fp16


def inputs(family, shape, cfg, seed, half=False):
    """(x1, x2, go) host tensors, float32 or fp16.  randn: N(0,1); offset: 100 + N(0,1); alternating: x2 = +-x1 over c, the
    zero-displacement sum cancels to the last channel while A stays large; tiny / huge: N(0,1) times 1e-15 / 1e+15."""
    B, C, H, W = shape
    _, _, ds, oH, oW = geometry(H, W, cfg)
    g = torch.Generator().manual_seed(seed)
    x1, x2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    go = torch.randn(B, ds * ds, oH, oW, generator=g)
    if family == "offset":
        x1, x2 = x1 + 100.0, x2 + 100.0
    elif family == "alternating":
        x2 = x1 * (1.0 - 2.0 * (torch.arange(C) % 2)).view(1, C, 1, 1)
        go = go * (1.0 - 2.0 * (torch.arange(ds * ds) % 2)).view(1, -1, 1, 1)
    elif family in ("tiny", "huge"):
        s = 1e-15 if family == "tiny" else 1e15
        x1, x2, go = x1 * s, x2 * s, go * s
    else:
        assert family == "randn"
    if half:
        assert family in HALF_FAMILIES
        return x1.half(), x2.half(), go.half()
    return x1, x2, go


def plant_nonfinite(x1, x2, go):
    """Copies with one +inf, one -inf and one NaN in each of x1, x2 and grad_out: one in a corner, one beside the 16-texel tile
    seam (x = 15 | 16, where the image is that wide) and one in the interior."""
    x1, x2, go = x1.clone(), x2.clone(), go.clone()
    vals = (float("inf"), float("-inf"), float("nan"))
    for n, t in enumerate((x1, x2, go)):
        B, C, H, W = t.shape
        seam = min(15 + n % 2, W - 1)
        spots = [(0, 0, 0, 0), (B - 1, C // 2, H // 2, seam), (B - 1, C - 1, max(H // 2 - 1, 0), W // 2)]
        if n == 1:
            spots[0] = (0, C - 1, H - 1, W - 1)
        for q, (bb, c, y, x) in enumerate(spots):
            t[bb, c, y, x] = vals[(q + n) % 3]
    return x1, x2, go


# ---- float32 emulation of the kernels' orders, for the host test -------------------------------------------------------------
def fma32(a, b, acc):
    """float32 fma: the product of two float32 is exact in float64; the sum rounds to float64 (relative 2^-53) and then to
    float32 -- the fused result except on a double-rounding tie, 2^-29 of a float32 ulp away from it."""
    return (a.double() * b.double() + acc.double()).float()


def chain32(av, bv, ks):
    """fma chain over the first dimension of av, bv (float32) in the order ks, from +0."""
    acc = torch.zeros_like((av[0] * bv[0]))
    for k in ks:
        acc = fma32(av[k], bv[k], acc)
    return acc


def emulate_forward32(x1, x2, md, s2, order):
    """The fast configuration (k = 1, s1 = 1, pad = md) in float32.  order 'ascending': one fma chain over c (the scalar and the
    general kernels); 'pipe': the matrix-pipe kernel's four interleaved chains -- chain q takes the channel groups of four
    g = q, q + 4, ... (each group taken as four fmas in ascending c) -- added pairwise (a0 + a1) + (a2 + a3)."""
    B, C, H, W = x1.shape
    dr = md // s2
    x1, x2p = x1.float(), F.pad(x2.float(), [md] * 4)
    a = x1.permute(1, 0, 2, 3).unsqueeze(2)   # [C, B, 1, H, W]
    inv = torch.tensor(1.0) / torch.tensor(float(C))
    offs = [(md + tj * s2, md + ti * s2) for tj in range(-dr, dr + 1) for ti in range(-dr, dr + 1)]
    b = torch.stack([x2p[:, :, y0:y0 + H, x0:x0 + W] for y0, x0 in offs], 2).permute(1, 0, 2, 3, 4)   # [C, B, ds ds, H, W]
    if order == "ascending":
        return chain32(a, b, range(C)) * inv
    assert order == "pipe"
    groups = range((C + 3) // 4)
    s = [chain32(a, b, [c for gq in groups if gq % 4 == q for c in range(4 * gq, min(4 * gq + 4, C))]) for q in range(4)]
    return ((s[0] + s[1]) + (s[2] + s[3])) * inv


def emulate_backward32(x1, x2, go, md, s2):
    """The fast backward in float32: per (pixel, channel) one fma per displacement in ascending d, then times 1/C."""
    B, C, H, W = x1.shape
    dr = md // s2
    x1p, x2p, gop = F.pad(x1.float(), [md] * 4), F.pad(x2.float(), [md] * 4), F.pad(go.float(), [md] * 4)
    g1, g2 = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    d = 0
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            dy, dx = tj * s2, ti * s2
            g1 = fma32(go[:, d:d + 1].float(), x2p[:, :, md + dy:md + dy + H, md + dx:md + dx + W], g1)
            g2 = fma32(gop[:, d:d + 1, md - dy:md - dy + H, md - dx:md - dx + W], x1p[:, :, md - dy:md - dy + H, md - dx:md - dx + W], g2)
            d += 1
    inv = torch.tensor(1.0) / torch.tensor(float(C))
    return g1 * inv, g2 * inv
