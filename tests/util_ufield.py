"""Shared by tests/test_ufield_host.py and tests/test_ufield_gpu.py: a reference of the uncertainty-field collapse
(pdepth_ufield_f32, csrc/ufield.hip; oracle.ref_cpu.gen_ufield) that decides every mask exactly and sums the plane in float64,
the bound the plane is held to, the comparison both files make, and the case table.

The masks of the collapse are comparisons of float32 values that IEEE operations derive from the depth map: the row of the
pixel minus cy, divided by fy, times the depth, against the band; the depth against the range; the depth against the column
minimum -+ 1.  Given the depth map itself -- the caller supplies it: the oracle's on the host, ops.dpv_expect's on the GPU,
which is bit for bit what launch_ufield computes -- numpy repeats those operations and gets the same bits, so no column has
to be left out because "a pixel near a threshold may flip".  What remains float arithmetic with a free order of summation is
the plane, which is summed here in float64 and compared under plane_bound(H)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


# ---- the sampling grid -------------------------------------------------------------------------------------------------------
def nearest_src(n, shift, sampled):
    """int64 [n]: source index of destination index i under the reference's nearest sampling of a shift by `shift` pixels,
    -1 outside the image.  convert_flowfield (utils/img_utils.py:170-176) builds the grid with the (size - 1) convention,
    grid_sample un-normalises it with align_corners=False: float32 op for op, the fma as a float64 product and sum rounded
    once to float32 (the product of two float32 is exact in float64).  sampled = (unc_ang != 0): the reference clones instead
    of sampling when it is false, and the function is the identity."""
    i = np.arange(n, dtype=np.int64)
    if not sampled:
        return i
    step = f32(2.0) / f32(n - 1)
    g = (f32(-1.0) + i.astype(f32) * step) - f32(shift) * step
    pos = ((g + f32(1.0)).astype(np.float64) * np.float64(f32(n) / f32(2.0)) + np.float64(-0.5)).astype(f32)
    r = np.rint(pos)
    inside = (r >= 0) & (r < n)
    return np.where(inside, np.where(inside, r, 0).astype(np.int64), -1)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def oob_depth(d_candi, bv_log):
    """The depth of rows shifted in from outside: E[d] of the zero padding, exp(0) = 1 per plane for a log-DPV -- the float32
    sum of the candidates as ops.ufield forms it (torch's float32 sum on the host) -- else 0."""
    if not bv_log:
        return f32(0.0)
    return f32(float(torch.from_numpy(np.ascontiguousarray(np.asarray(d_candi), dtype=f32)).sum()))


def prob64(vol, bv_log):
    """float64 probabilities of a float32 volume: exp in float64 for a log-DPV."""
    v = np.asarray(vol, dtype=np.float64)
    return np.exp(v) if bv_log else v


def depth64(vol, d_candi, bv_log):
    """E[d] [H,W] in float64 over the float32 candidates."""
    d = np.asarray(d_candi).astype(f32).astype(np.float64)
    return np.tensordot(d, prob64(vol, bv_log), axes=(0, 0))


def _ulp32(t):
    return np.spacing(np.abs(f32(t))).astype(np.float64)


def _near(v64, t32):
    """|v - t| <= 2 ulp32(t).  A threshold of exactly 0 is never near: that comparison is decided by the operand's sign, which
    no rounding of a product or a quotient changes."""
    t32 = np.asarray(t32, dtype=f32)
    return (np.abs(v64 - t32.astype(np.float64)) <= 2 * _ulp32(t32)) & (t32 != 0)


WRONG = ("back_shift_plus", "sx_identity", "last_row_dropped", "last_segment_dropped", "oob_zero", "quash_unmasked")


def ufield_reference(vol, d_candi, intr, mask, bv_log, unc_ang, z_start, z_end, min_depth, quash, depth_pred, p64=None,
                     wrong=None):
    """Per item.  vol [D,H,W] float32, intr [3,3], mask [H,W] | None, depth_pred [H,W] float32 (the depth map the masks are
    decided on) -> dict(plane [D,W] float64, depth_zero [H,W] float32, zm [H,W] float32 (the mask of the shifted points, ax
    its column sums), near [H,W] bool: pixels where the float64 value of Y, or of an operand of the quash window, is within
    2 ulp32 of the threshold it is compared with (the depth is an input, compared as it is: it is flagged by the same rule).
    p64 = prob64(vol, bv_log) if the caller has it.  wrong: one of WRONG, a deliberately wrong reference (test_ufield_host.py
    shows that the cases tell each from the right one)."""
    assert wrong is None or wrong in WRONG
    vol = np.asarray(vol)
    D, H, W = vol.shape
    depth_pred = np.asarray(depth_pred, dtype=f32)
    assert depth_pred.shape == (H, W)
    intr = np.asarray(intr, dtype=f32)
    sampled = unc_ang != 0
    sy = nearest_src(H, unc_ang, sampled)
    sx = nearest_src(W, 0.0, sampled and wrong != "sx_identity")
    sy_back = nearest_src(H, unc_ang if wrong == "back_shift_plus" else -unc_ang, sampled)
    oob = f32(0.0) if wrong == "oob_zero" else oob_depth(d_candi, bv_log)

    def gather(img, iy, ix, outside):
        inb = (iy >= 0)[:, None] & (ix >= 0)[None, :]
        return np.where(inb, img[np.maximum(iy, 0)[:, None], np.maximum(ix, 0)[None, :]], f32(outside)).astype(f32)

    d = gather(depth_pred, sy, sx, oob)
    cy, fy = intr[1, 2], intr[1, 1]
    yf = (np.arange(H, dtype=f32) - cy) / fy                               # float32: the correctly rounded quotient
    Y = yf[:, None] * d
    zs, ze, mind, maxd = f32(z_start), f32(z_end), f32(min_depth), f32(99.0)
    zm = (~((Y > ze) | (Y < zs) | (d > maxd) | (d < mind))).astype(f32)
    Y64 = (np.arange(H, dtype=np.float64) - np.float64(cy))[:, None] / np.float64(fy) * d.astype(np.float64)
    near = _near(Y64, ze) | _near(Y64, zs) | _near(d.astype(np.float64), maxd) | _near(d.astype(np.float64), mind)
    if mask is not None:
        zm = zm * gather(np.asarray(mask, dtype=f32), sy, sx, 0.0)
    if quash:                                                              # oracle/ref_cpu.py:283-287
        cleaned = d.copy() if wrong == "quash_unmasked" else d * zm
        cleaned[cleaned == 0] = f32(1000.0)
        min_col = cleaned.min(axis=0)
        lo, hi = min_col - f32(1.0), min_col + f32(1.0)
        zm = zm * ((cleaned > lo) & (cleaned < hi)).astype(f32)
        c64 = cleaned.astype(np.float64)
        near = near | _near(c64, np.broadcast_to(lo, cleaned.shape)) | _near(c64, np.broadcast_to(hi, cleaned.shape))
    ax = zm.astype(np.float64).sum(axis=0)                                 # (exact: multiples of 1/2 far below 2^24)
    zb = gather(zm, sy_back, sx, 0.0)
    if wrong == "last_row_dropped":
        zb[H - 1:] = 0
    elif wrong == "last_segment_dropped":
        zb[H - (H + 7) // 8:] = 0
    depth_zero = depth_pred * zb
    p = prob64(vol, bv_log) if p64 is None else p64
    with np.errstate(invalid="ignore", divide="ignore"):
        plane = (p * zb.astype(np.float64)[None]).sum(axis=1) / ax[None, :]
    return {"plane": plane, "depth_zero": depth_zero, "zm": zm, "ax": ax, "near": near}


def plane_bound(H):
    """Relative to the float64 value (plus 1e-36 absolute).  Every term is non-negative; a column is summed by at most
    ceil(H / 8) sequential adds plus 15 combining adds, each one rounding; expf is at most 2 ulp; the product with a
    non-binary mask is one rounding and the final divide is one: (ceil(H / 8) + 24) 2^-24 covers them with a few to spare.
    A dropped or doubled row among N qualifying rows is off by about 1 / N, a wrong mask by more."""
    return (math.ceil(H / 8) + 24) * 2.0 ** -24


ABS_BOUND = 1e-36


def compare(plane, depth_zero, ref, H, bound_factor=1.0, skip_columns=None):
    """The comparison both files make, of a float32 (or float64) result against ufield_reference's: -> dict(dz_diff: pixels
    of depth_zero that are not bit-equal, nan_diff: entries of the plane whose NaN-ness differs, worst: the largest
    |got - f64| / (plane_bound |f64| + 1e-36) over the finite entries, over: entries beyond it).  bound_factor 2 where the
    other side is itself a float32 sum (the oracle).  skip_columns: bool [W], columns left out (none, unless the caller has
    shown that numpy cannot follow a correct kernel there)."""
    got = np.asarray(plane, dtype=np.float64)
    want = ref["plane"]
    assert got.shape == want.shape, (got.shape, want.shape)
    dz = np.asarray(depth_zero, dtype=f32)
    assert dz.shape == ref["depth_zero"].shape
    keep = np.ones(want.shape[1], dtype=bool) if skip_columns is None else ~np.asarray(skip_columns, dtype=bool)
    dz_diff = np.ascontiguousarray(dz).view(np.uint32) != np.ascontiguousarray(ref["depth_zero"]).view(np.uint32)
    nan_diff = np.isnan(got) != np.isnan(want)
    both = ~np.isnan(got) & ~np.isnan(want)
    with np.errstate(invalid="ignore"):
        ratio = np.where(both, np.abs(got - want) / (plane_bound(H) * bound_factor * np.abs(want) + ABS_BOUND), 0.0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                       # inf against inf - or anything else - is no match
    ratio[both & (got == want)] = 0.0
    return {"dz_diff": int(dz_diff[:, keep].sum()), "nan_diff": int(nan_diff[:, keep].sum()),
            "worst": float(ratio[:, keep].max()) if keep.any() else 0.0, "over": int((ratio[:, keep] > 1.0).sum()),
            "bad_columns": np.flatnonzero((dz_diff.any(axis=0) | nan_diff.any(axis=0) | (ratio > 1.0).any(axis=0)))}


def matches(c):
    return c["dz_diff"] == 0 and c["nan_diff"] == 0 and c["over"] == 0


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# name -> (D, H, W, seed).  What each is for is in the table of test_ufield_gpu.py's docstring.
UFIELD_CASES = {
    "two_columns": (5, 9, 2, 7101),            # smallest width; even W loses its last column when shifted
    "two_rows": (7, 2, 13, 7102),              # H < 8: empty row segments; a shift beyond H
    "scalar_ragged": (33, 30, 65, 7103),       # scalar collapse, the second 64-column block holds one column, D % 4 = 1
    "scalar_even": (8, 257, 66, 7104),         # scalar, even W, second trip of the mask kernel's 256-row loop
    "vec4_odd_planes": (9, 33, 260, 7105),     # vec4, last plane pair half empty, second 256-column block holds one quad
    "vec4_wide_short": (2, 16, 256, 7106),     # vec4, exactly one block, exactly one row per segment
    "vec4_short": (64, 12, 132, 7107),         # vec4 with 8 < H < 16: empty segments
    "tall_narrow": (4, 513, 4, 7108),          # third trip of the mask loop, one quad
    "oob_depth_in_range": (3, 300, 8, 7109),   # sum(d) = 33 < 99: rows shifted in from outside qualify
    "d_over_128": (130, 12, 40, 7110),         # inner expectation on the D > 128 kernel
    "model_rows": (64, 256, 68, 7111),         # the model's row count at the narrowest vec4 width with an odd quad count
    "unaligned": (8, 20, 64, 7112),            # the volume one float into a flat buffer: scalar collapse and expectation
}
CASE_NAMES = tuple(UFIELD_CASES)
SCALAR_CASES = ("two_columns", "two_rows", "scalar_ragged", "scalar_even", "unaligned")   # W % 4 != 0 or unaligned
BRANCHES = ((3.0, True), (0.0, False))          # (min_depth, quash): the cfgx / ilim branch and the kitti branch
MASKS = ("none", "random", "columns_zeroed")
BATCH_CASES = ("scalar_ragged", "vec4_odd_planes", "tall_narrow")
BATCH_CY_SHIFT, BATCH_FY_SCALE = (0.0, 1.7, -2.4), (1.0, 0.8, 1.3)
# the B = 3 calls: a quashed log-DPV shifted by 5 rows, unquashed probabilities shifted by -3
BATCH_VARIANTS = ((5, True, BRANCHES[0], "none"), (-3, False, BRANCHES[1], "none"))

# oob_depth_in_range: with the common principal point (cy = H / 2 - 0.2, fy = 0.8 H) the rows shifted in from outside are
# the outermost ones, |y - cy| / fy = 0.62, and 0.62 * 33 m = 20 m lies far outside the band [-1.65, 2.97] m: they could
# never qualify and the case would not exercise what it is named for.  Its principal point sits on row 2.8 instead, where
# the rows a shift of 5 brings in (y < 5) are in the band.
# one_row: its only row a tenth of a pixel above the principal point, so that most of its 19 pixels are in the band.
CASE_CY = {"oob_depth_in_range": 2.8, "one_row": 0.1}

_CACHE = {}


def cached(key, make):
    """References are computed once and shared: treat what comes back as read-only."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def candidates(D):
    return np.linspace(3.0, 40.0, D) if D > 3 else np.array((4.0, 9.0, 20.0)[:D])


def intrinsics(name, H, W):
    cy = CASE_CY.get(name, H / 2.0 - 0.2)
    return torch.tensor([[0.9 * W, 0.0, W / 2.0 + 0.3], [0.0, 0.8 * H, cy], [0.0, 0.0, 1.0]])


def _make_item(name, D, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    logdpv = F.log_softmax(torch.randn(D, H, W, generator=g) * 3, dim=0)
    random = (torch.rand(H, W, generator=g) < 0.7).float()
    zeroed = random.clone()
    zeroed[:, 0] = 0
    zeroed[:, W // 2] = 0
    halves = torch.randint(0, 3, (H, W), generator=g).float() / 2          # {0, 0.5, 1}
    d_candi = candidates(D)
    mean = float(np.mean(d_candi))
    z_start, span = -0.15 * mean, 0.42 * mean
    return {"name": name, "shape": (D, H, W), "log": logdpv, "prob": torch.exp(logdpv), "d_candi": d_candi,
            "intr": intrinsics(name, H, W), "z_start": z_start, "span": span, "z_end": z_start + span,   # (as gen_ufield adds them)
            "masks": {"none": None, "random": random, "columns_zeroed": zeroed, "halves": halves}}


def case(name):
    """dict(shape, log / prob [D,H,W], d_candi float64 [D], intr [3,3], z_start, span, z_end, masks {name: [H,W] | None})."""
    D, H, W, seed = UFIELD_CASES[name]
    return cached(("case", name), lambda: _make_item(name, D, H, W, seed))


def one_column_case():
    """W = 1 is legal without a shift (the reference's grid of a shift divides by size - 1)."""
    return cached(("case", "one_column"), lambda: _make_item("one_column", 6, 19, 1, 7120))


def one_row_case():
    """H = 1 likewise."""
    return cached(("case", "one_row"), lambda: _make_item("one_row", 6, 1, 19, 7121))


def batch_items(name):
    """Three seeds of a case for one B = 3 call: intrinsics and masks differ per item (random, all ones, all zero)."""
    D, H, W, seed = UFIELD_CASES[name]

    def make():
        items = [case(name)] + [_make_item(name, D, H, W, seed + 100 * b) for b in (1, 2)]
        out = []
        for b, it in enumerate(items):
            it = dict(it)
            intr = it["intr"].clone()
            intr[1, 2] += BATCH_CY_SHIFT[b]
            intr[1, 1] *= BATCH_FY_SCALE[b]
            it["intr"] = intr
            it["mask"] = (it["masks"]["random"], torch.ones(H, W), torch.zeros(H, W))[b]
            out.append(it)
        return out
    return cached(("batch", name), make)


def variants(name):
    """[(unc_ang, bv_log, (min_depth, quash), mask name)] of a case: shifts 0, 5, -3 (two_rows also H + 2, scalar_ragged also
    2.5), both volume forms, both branches, the three masks; scalar_ragged once more with the non-binary mask."""
    H = UFIELD_CASES[name][1]
    angs = [0, 5, -3] + ([H + 2] if name == "two_rows" else []) + ([2.5] if name == "scalar_ragged" else [])
    out = [(a, bv, br, m) for a in angs for bv in (True, False) for br in BRANCHES for m in MASKS]
    if name == "scalar_ragged":
        out.append((5, True, BRANCHES[0], "halves"))
    return out


def degenerate(name, variant):
    """A shift at or beyond H: nothing of the image is left, no pixel can qualify."""
    return abs(variant[0]) >= UFIELD_CASES[name][1]


def variant_id(v):
    return "ang%g/%s/mind%g%s/%s" % (v[0], "log" if v[1] else "prob", v[2][0], "+quash" if v[2][1] else "", v[3])


def volume(c, bv_log):
    return c["log"] if bv_log else c["prob"]


def case_p64(c, bv_log):
    return cached(("p64", c["name"], id(c["log"]), bv_log), lambda: prob64(volume(c, bv_log).numpy(), bv_log))


def reference(c, variant, depth_pred, mask=None, intr=None, wrong=None):
    """ufield_reference of a case dict (or batch item) and a variant, on the depth map given."""
    ang, bv_log, (mind, quash), mname = variant
    m = c["masks"][mname] if mask is None else mask
    return ufield_reference(volume(c, bv_log).numpy(), c["d_candi"], (c["intr"] if intr is None else intr).numpy(),
                            None if m is None else m.numpy(), bv_log, ang, c["z_start"], c["z_end"], mind, quash,
                            np.asarray(depth_pred), p64=case_p64(c, bv_log), wrong=wrong)
