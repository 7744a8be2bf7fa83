"""SSIM restated from its definition, for the tests of ops.ssim (tests/test_ssim_host.py, tests/test_ssim_gpu.py).

  ssim_parts / ssim_dist   the forward, written from the formula (window sums by explicit shifted slices, no pooling op), in the
                           dtype of its inputs: float64 = the tests' reference, float32 = "the torch composition of the same formula"
  ssim_grads               the gradients by the per-window coefficient maps P, P', Q, R (include/pdepth.h), no autograd
  make_base / case_inputs  the inputs of the fixture's cases (tests/golden/make_golden_ssim.py)
  cases                    tests/golden/g23_ssim.npz, by case name: inputs and the reference's float32 results
"""
import os

import numpy as np
import torch

C1, C2 = 0.01 ** 2, 0.03 ** 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_ssim.npz")
MDS = (1, 2, 3)
KINDS = ("indep", "noisy", "masked", "same", "const", "one")
EDGE = 1e-6   # an element whose float64 (1 - S) / 2 is this close to 0 or 1 without being on it may take either side of the clamp


def window_sum(t, md):
    """Sum over every (2 md + 1)^2 window of the last two dimensions: [...,H,W] -> [...,H-2md,W-2md]."""
    k = 2 * md + 1
    H, W = t.shape[-2:]
    out = None
    for dy in range(k):
        for dx in range(k):
            part = t[..., dy:H - 2 * md + dy, dx:W - 2 * md + dx]
            out = part if out is None else out + part
    return out


def ssim_parts(x, y, md):
    """dict of the per-window quantities: m_x, m_y, A1, A2, B1, B2, S and raw = (1 - S) / 2 before the clamp."""
    # n as a tensor: a quotient by a Python number is, on the device, a product with its rounded reciprocal (1 / 9 is not a
    # float), which is not the formula's "sum divided by n"
    n = x.new_full((), float((2 * md + 1) ** 2))
    mx, my = window_sum(x, md) / n, window_sum(y, md) / n
    sx = window_sum(x * x, md) / n - mx * mx
    sy = window_sum(y * y, md) / n - my * my
    sxy = window_sum(x * y, md) / n - mx * my
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sx + sy + C2
    S = A1 * A2 / (B1 * B2)
    return {"mx": mx, "my": my, "A1": A1, "A2": A2, "B1": B1, "B2": B2, "S": S, "raw": (1 - S) / 2}


def ssim_dist(x, y, md):
    return ssim_parts(x, y, md)["raw"].clamp(0, 1)


def _spread(t, md, H, W):
    """Transpose of window_sum: [...,H-2md,W-2md] per-window values -> [...,H,W], each pixel the sum over the windows that contain it."""
    k = 2 * md + 1
    out = t.new_zeros(t.shape[:-2] + (H, W))
    for dy in range(k):
        for dx in range(k):
            out[..., dy:H - 2 * md + dy, dx:W - 2 * md + dx] += t
    return out


def ssim_grads(x, y, g_out, md, flip=None):
    """(g_x, g_y) by the coefficient maps.  A window passes the gradient on 0 <= (1 - S) / 2 <= 1, edges included (torch.clamp's
    rule); flip: a boolean map of windows whose decision is inverted (the other rule, for windows too close to an edge to call)."""
    p = ssim_parts(x, y, md)
    n = float((2 * md + 1) ** 2)
    H, W = x.shape[-2:]
    raw = p["raw"]
    passes = (raw >= 0) & (raw <= 1)
    if flip is not None:
        passes = passes ^ flip
    G = -0.5 * g_out * passes.to(g_out.dtype)
    mx, my, A1, A2, B1, B2, S = (p[k] for k in ("mx", "my", "A1", "A2", "B1", "B2", "S"))
    P = 2 * my * (A2 - A1) / (B1 * B2) - S * (2 * mx / B1 - 2 * mx / B2)
    Pp = 2 * mx * (A2 - A1) / (B1 * B2) - S * (2 * my / B1 - 2 * my / B2)
    Q = -2 * S / B2
    R = 2 * A1 / (B1 * B2)
    sP, sPp, sQ, sR = (_spread(G * t, md, H, W) for t in (P, Pp, Q, R))
    return (sP + sQ * x + sR * y) / n, (sPp + sQ * y + sR * x) / n


def near_edge(raw64):
    """Elements whose float64 (1 - S) / 2 lies within EDGE of 0 or 1 without being on it."""
    return ((raw64 != 0) & (raw64.abs() < EDGE)) | ((raw64 != 1) & ((raw64 - 1).abs() < EDGE))


SHAPE = (2, 3, 21, 37)
CONST = np.float32(0.3)


def make_base():
    """The random arrays the cases are built from, float32, from frozen streams: {f"md{md}_{name}": array}.  The cases of one md
    share x, the mask and g_out (random float32 does not compress; the fixture stores each array once)."""
    out = {}
    for md in MDS:
        rng = np.random.RandomState(2310 + md)   # (chosen so that no window of a case lies within EDGE of a clamp edge off it)
        k = 2 * md + 1
        x = rng.uniform(0, 1, SHAPE).astype(np.float32)
        m = (rng.uniform(0, 1, (SHAPE[0], 1) + SHAPE[2:]) < 0.8).astype(np.float32)
        m[:, :, :SHAPE[2] // 3] = 0
        base = {"x": x, "indep": rng.uniform(0, 1, SHAPE).astype(np.float32),
                "noisy": np.clip(x + np.float32(0.05) * rng.standard_normal(SHAPE).astype(np.float32), 0, 1).astype(np.float32),
                "mask": m, "g_out": rng.standard_normal(SHAPE[:2] + (SHAPE[2] - 2 * md, SHAPE[3] - 2 * md)).astype(np.float32),
                "one_x": rng.uniform(0, 1, (1, 3, k, k)).astype(np.float32), "one_y": rng.uniform(0, 1, (1, 3, k, k)).astype(np.float32),
                "one_g_out": rng.standard_normal((1, 3, 1, 1)).astype(np.float32)}
        out.update({f"md{md}_{name}": v for name, v in base.items()})
    return out


def case_inputs(base, kind, md):
    """(x, y, g_out) of a case from the base arrays (make_base() or the fixture)."""
    b = lambda name: np.asarray(base[f"md{md}_{name}"])
    x, m = b("x"), b("mask")
    if kind == "one":
        return b("one_x"), b("one_y"), b("one_g_out")
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
