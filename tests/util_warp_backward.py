"""Shared by tests/test_warp_backward_host.py and tests/test_warp_backward_gpu.py: the float64 autograd oracle of
warp_feature's backward and the bound a float32 backward is held to.

The oracle is util_warps.warp_feature_exact64 on a float64 leaf (the float64 gather at the oracle's float32 positions).  With an
upstream gradient g and the in-bounds taps' weights w:
    g64[t] = sum_i g_i w_i          the gradient,
    A[t]   = sum_i |g_i| w_i        the same with |g| as upstream (the weights are >= 0),
    n[t]   = the number of in-bounds taps that land on texel t (ones scattered at the oracle's taps).
A float32 backward -- the reference's own, the float atomics or the integer sum -- is held to
    |g32 - g64| <= (4 + n) eps32 A,        and to exactly 0 where A == 0:
each q_i = fl(g_i w_i) carries at most 4 roundings (at most 3 in the weight, 1 in the product): at most 2 eps32 |q_i|; a sum of n
terms in any order adds at most (n - 1) eps32 / 2 sum|q|; the integer path adds below 2^-59 N M per contribution and one final
rounding.  In total at most (2 + n / 2) eps32 A; the bound is twice that."""
import torch

import util_warps as U

EPS32 = U.EPS32
SEED = 7


def upstream(name):
    """g_out ~ N(0, 1) [B,V,D,H,W] float32 of a case, fixed seed."""
    shape = U.warp_feature_case(name)["src"].shape
    return U.cached(("wfb_gout", name), lambda: torch.randn(tuple(shape), generator=torch.Generator().manual_seed(SEED)))


def positions(name):
    return U.cached(("wfb_pos", name), lambda: U.oracle_positions(U.warp_feature_case(name)))


def tap_indices(ix, iy, H, W):
    """-> [(inside bool, flat texel index int64)] of the four taps, each shaped like ix."""
    fin, x0, y0, _, _ = U._taps(ix, iy, H, W)
    out = []
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        inside = fin & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        out.append((inside, yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)))
    return out


def tap_counts(ix, iy):
    """n [B,V,D,H,W] float64: in-bounds taps per texel of each (b,v,k) image."""
    B, V, D, H, W = ix.shape
    n = torch.zeros(B * V * D, H * W, dtype=torch.float64)
    for inside, idx in tap_indices(ix.reshape(B * V * D, -1), iy.reshape(B * V * D, -1), H, W):
        n.scatter_add_(1, idx, inside.double())
    return n.reshape(B, V, D, H, W)


def oracle_grads(batch, pos, g_out, src=None):
    """(g64, A) float64 in the shape of src (default batch['src']): autograd through warp_feature_exact64."""
    leaf = (batch["src"] if src is None else src).double().clone().requires_grad_(True)
    exact, fin = U.warp_feature_exact64(batch, src=leaf, positions=pos)
    assert bool(fin.all()), "every position of the cases is finite"
    g64, = torch.autograd.grad(exact, leaf, g_out.double(), retain_graph=True)
    A, = torch.autograd.grad(exact, leaf, g_out.double().abs())
    return g64, A


def reference(name):
    """dict(g_out, g64, A, n, bound) of a case, cached: treat as read-only."""
    def make():
        b, pos, g = U.warp_feature_case(name), positions(name), upstream(name)
        g64, A = oracle_grads(b, pos, g)
        n = tap_counts(*pos)
        return {"g_out": g, "g64": g64, "A": A, "n": n, "bound": (4 + n) * EPS32 * A}
    return U.cached(("wfb_ref", name), make)


def check(got, ref, what, bound=None, want=None):
    """Every texel: |got - g64| <= bound, exactly 0 where A == 0.  Returns the worst error / bound (for the record)."""
    want = ref["g64"] if want is None else want
    bound = ref["bound"] if bound is None else bound
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    zero = bound == 0
    assert bool((got[zero] == 0).all()), f"{what}: a texel no tap reaches is not exactly 0"
    err = (got - want).abs()
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    print(f"{what}: worst error / bound = {ratio:.3f}, texels no tap reaches: {int(zero.sum())} of {zero.numel()}")
    assert bool((err <= bound).all()), f"{what}: worst error / bound = {ratio:.3f}"
    return ratio
