"""The ternary census distance restated from its definition, for the tests of ops.ternary (tests/test_ternary_host.py,
tests/test_ternary_gpu.py).

  ternary_dist             the forward, written from the formula as a pad, a shift and a subtraction per offset (no conv), in the
                           dtype of its inputs: float64 = the tests' reference, float32 = "the torch composition of the same formula"
  ternary_grads            the gradients of (ternary_dist * g_out).sum() by autograd, in the dtype of the inputs
  ternary_grads_analytic   the same gradients from the closed form of include/pdepth.h, no autograd
  make_base / case_inputs  the inputs of the fixture's cases (tests/golden/make_golden_ternary.py)
  cases                    tests/golden/g26_ternary.npz, by case name: inputs and the reference's float32 results
  tile                     (width, height) of the kernels' tile, read from csrc/ternary.hip
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g26_ternary.npz")
KERNELS = os.path.join(os.path.dirname(HERE), "probabilistic-depth_amd", "csrc", "ternary.hip")
MDS = (1, 2, 3)
KINDS = ("indep", "noisy", "masked", "same", "const", "one")


def gray255(im):
    """[B,3,H,W] -> [B,H,W]: the grayscale times 255."""
    return (im[:, 0] * 0.2989 + im[:, 1] * 0.5870 + im[:, 2] * 0.1140) * 255


def _offsets(md):
    return [(dy, dx) for dy in range(2 * md + 1) for dx in range(2 * md + 1)]


def _shifted(I, md):
    """I(p+o) for every offset o of the patch, zero padding outside the image: [B,H,W] -> [B,K^2,H,W]."""
    H, W = I.shape[-2:]
    P = F.pad(I, [md] * 4)
    return torch.stack([P[:, dy:dy + H, dx:dx + W] for dy, dx in _offsets(md)], dim=1)


def inner_mask(t, md):
    """1 where a pixel is at least md from every border: [..,H,W] of t's dtype."""
    m = torch.zeros(t.shape[-2:], dtype=t.dtype, device=t.device)
    m[md:t.shape[-2] - md, md:t.shape[-1] - md] = 1
    return m


def ternary_dist(x, y, md):
    """x, y [B,3,H,W] -> [B,1,H,W]."""
    def transform(im):
        I = gray255(im)
        t = _shifted(I, md) - I.unsqueeze(1)
        return t / torch.sqrt(0.81 + t * t)

    e = transform(x) - transform(y)
    d = e * e
    h = d / (0.1 + d)
    n = x.new_full((), float((2 * md + 1) ** 2))   # (a tensor: a quotient by a Python number is a product with its reciprocal on the device)
    return (h.sum(1, keepdim=True) / n) * inner_mask(x, md)


def ternary_grads(x, y, g_out, md):
    """(g_x, g_y) of (ternary_dist(x, y, md) * g_out).sum() by autograd."""
    a, b = x.detach().clone().requires_grad_(True), y.detach().clone().requires_grad_(True)
    (ternary_dist(a, b, md) * g_out).sum().backward()
    return a.grad, b.grad


def ternary_grads_analytic(x, y, g_out, md):
    """(g_x, g_y) by g_I(p) = -sum_o (G(p) + G(p+o)) dh/dt of the pair (p, p+o), G = g_out mask / K^2, 0 outside the image."""
    K2 = float((2 * md + 1) ** 2)
    I, Ip = gray255(x), gray255(y)
    t, tp = _shifted(I, md) - I.unsqueeze(1), _shifted(Ip, md) - Ip.unsqueeze(1)
    u, up = 0.81 + t * t, 0.81 + tp * tp
    s, sp = torch.sqrt(u), torch.sqrt(up)
    e = t / s - tp / sp
    a = 0.2 * e / (0.1 + e * e) ** 2
    G = g_out[:, 0] * inner_mask(x, md) / K2
    w = G.unsqueeze(1) + _shifted(G, md)
    gI, gIp = -(w * a * 0.81 / (u * s)).sum(1), (w * a * 0.81 / (up * sp)).sum(1)
    coef = x.new_tensor([0.2989, 0.5870, 0.1140]).reshape(1, 3, 1, 1) * 255
    return gI.unsqueeze(1) * coef, gIp.unsqueeze(1) * coef


SHAPE = (2, 3, 21, 37)
CONST = np.float32(0.3)


def make_base():
    """The random arrays the cases are built from, float32, from frozen streams.  The cases of every md share x, the second images,
    the mask and g_out (random float32 does not compress; the fixture stores each array once); the one-interior-pixel shape depends
    on md."""
    rng = np.random.RandomState(2610)
    x = rng.uniform(0, 1, SHAPE).astype(np.float32)
    m = (rng.uniform(0, 1, (SHAPE[0], 1) + SHAPE[2:]) < 0.8).astype(np.float32)
    m[:, :, :SHAPE[2] // 3] = 0
    out = {"x": x, "indep": rng.uniform(0, 1, SHAPE).astype(np.float32),
           "noisy": np.clip(x + np.float32(0.05) * rng.standard_normal(SHAPE).astype(np.float32), 0, 1).astype(np.float32),
           "mask": m, "g_out": rng.standard_normal((SHAPE[0], 1) + SHAPE[2:]).astype(np.float32)}
    for md in MDS:
        k = 2 * md + 1
        out[f"md{md}_one_x"] = rng.uniform(0, 1, (1, 3, k, k)).astype(np.float32)
        out[f"md{md}_one_y"] = rng.uniform(0, 1, (1, 3, k, k)).astype(np.float32)
        out[f"md{md}_one_g_out"] = rng.standard_normal((1, 1, k, k)).astype(np.float32)
    return out


def case_inputs(base, kind, md):
    """(x, y, g_out) of a case from the base arrays (make_base() or the fixture)."""
    b = lambda name: np.asarray(base[name])
    if kind == "one":
        return b(f"md{md}_one_x"), b(f"md{md}_one_y"), b(f"md{md}_one_g_out")
    x, m = b("x"), b("mask")
    const = np.full(SHAPE, CONST, dtype=np.float32)
    pair = {"indep": lambda: (x, b("indep")), "noisy": lambda: (x, b("noisy")), "masked": lambda: (x * m, b("noisy") * m),
            "same": lambda: (x, x.copy()), "const": lambda: (const, const.copy())}[kind]()
    return pair[0], pair[1], b("g_out")


_cases = None


def cases():
    """name -> dict(md, x, y, g_out: the inputs; dist, g_x, g_y: the reference's float32 results) of the fixture, as numpy arrays."""
    global _cases
    if _cases is None:
        z = np.load(GOLDEN)
        _cases = {}
        for md in MDS:
            for kind in KINDS:
                x, y, g = case_inputs(z, kind, md)
                name = f"{kind}_md{md}"
                _cases[name] = {"md": md, "x": x, "y": y, "g_out": g, "dist": z[name + "_dist"], "g_x": z[name + "_g_x"],
                                "g_y": z[name + "_g_y"]}
    return _cases


def tile():
    """(TERN_TW, TERN_TH) of csrc/ternary.hip."""
    text = open(KERNELS).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("TERN_TW", "TERN_TH"))
