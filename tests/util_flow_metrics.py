"""Inputs of the flow-metrics fixture (tests/golden/g30_flow_metrics.npz), built the same way by the generator and by the tests
from numpy's frozen default_rng streams; the float64 statement of the formulas (metrics64, resize64); the derived bound.

The inputs are built so that the counts are decidable in float32.  With P the float64 resize of the rescaled prediction, the
truth is gt_uv = P + e, |e| drawn per pixel from U(0.1, 2.5) ("small") or U(3.5, 12) ("big") in a random direction.  |P| is
below 45 on most of the map (magnitudes U(0, 40) in any direction: a bilinear mix of such vectors stays below 40) and above 350
on a planted block (magnitudes U(360, 400) within 0.2 rad of one direction: a mix keeps at least 360 cos 0.2 = 352).  Where a
pixel's taps mix the two (45 <= |P| <= 350) only the small class is used.  Then a pixel with epe > 3 has
epe / |gt| >= 3.5 / 57 = 0.061 (|P| < 45) or <= 12 / 338 = 0.036 (|P| > 350), and no pixel has |epe - 3| < 0.5.  make_case
asserts that, with the margins |epe m - 3| >= 0.05 for every pixel and mask and |epe m / |gt| - 0.05| >= 0.005 wherever
epe m > 3 (the ratio decides nothing elsewhere): conditions on the inputs, not tolerances.  A seed that breaks one is changed."""
import numpy as np

B = 2
# name -> ((h, w) of the prediction, (H, W) of the truth)
CASES = {
    "same": ((9, 12), (9, 12)),            # identity: the bits of numpy's pred / w * W
    "up4": ((9, 12), (36, 48)),            # exact 4x, W % 4 == 0: the 16-byte path, seven workgroups with a partial one
    "odd_up": ((16, 32), (23, 61)),        # odd sizes, both axes up: the scalar path
    "down": ((16, 48), (10, 20)),          # both axes down (no antialiasing)
    "mixed": ((12, 40), (30, 24)),         # rows up, columns down
    "tiny": ((5, 7), (7, 13)),             # one partial workgroup; item 1: noc == valid
    "wide": ((32, 130), (128, 520)),       # 260 workgroups per item: the final pass's stride loop takes a second trip
}
FORMS = ("uv", "masks", "move")            # 2-channel truth, 4-channel truth, 4-channel truth + move mask
NOC_IS_VALID = ("tiny", 1)
NAMES = ("epe", "epe_noc", "epe_occ", "fl", "epe_move", "epe_static", "fl_move", "fl_static")
EPS32 = 2.0 ** -24


def _taps(n_out, n_in, align_corners):
    i = np.arange(n_out, dtype=np.float64)
    if align_corners:
        s = i * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
    else:
        s = (i + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(s).astype(np.int64)
    f = s - i0
    f[i0 < 0] = 0.0
    i0[i0 < 0] = 0
    f[i0 >= n_in - 1] = 0.0
    i0[i0 >= n_in - 1] = n_in - 1
    return i0, np.minimum(i0 + 1, n_in - 1), f


def resize64(x, size, align_corners=False):
    """[..., h, w] -> [..., H, W] in float64: half-pixel centres, x0 = floor(sx), x0 < 0 -> tap 0 alone, x0 >= w - 1 -> tap
    w - 1 alone (cv2.resize, INTER_LINEAR), or the coordinates of align_corners."""
    x = np.asarray(x, dtype=np.float64)
    (y0, y1, fy), (x0, x1, fx) = _taps(size[0], x.shape[-2], align_corners), _taps(size[1], x.shape[-1], align_corners)
    top = x[..., y0, :][..., :, x0] * (1 - fx) + x[..., y0, :][..., :, x1] * fx
    bot = x[..., y1, :][..., :, x0] * (1 - fx) + x[..., y1, :][..., :, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def rescale64(pred, size):
    """The rescaled prediction in float64: u / w * W, v / h * H on the float32 values."""
    p = np.asarray(pred, dtype=np.float64).copy()
    h, w = p.shape[-2:]
    p[..., 0, :, :] = p[..., 0, :, :] / w * size[1]
    p[..., 1, :, :] = p[..., 1, :, :] / h * size[0]
    return p


def flow_up64(pred, size, align_corners=False):
    return resize64(rescale64(pred, size), size, align_corners)


def _epe_terms(gt, pred):
    P = flow_up64(pred, gt.shape[-2:])
    g = np.asarray(gt, dtype=np.float64)
    epe = np.sqrt(((P - g[:2]) ** 2).sum(0))
    gmag = np.maximum(np.sqrt((g[:2] ** 2).sum(0)), 1e-10)
    return epe, gmag


def _bad(epe, m, gmag):
    return np.logical_and(epe * m > 3, epe * m / gmag > 0.05)


def metrics64(gt, pred, move=None):
    """One item: gt [2|4,H,W], pred [2,h,w] [, move [H,W]] (float32 values) -> (errors [8], counts [5], bad [3]) in float64;
    columns the inputs do not define are NaN (bad: -1)."""
    errors, counts, bad = np.full(8, np.nan), np.full(5, np.nan), np.full(3, -1.0)
    epe, gmag = _epe_terms(gt, pred)
    with np.errstate(invalid="ignore", divide="ignore"):
        if gt.shape[0] == 2:
            errors[0], counts[0] = epe.mean(), epe.size
            return errors, counts, bad
        valid, noc = np.float64(gt[2]), np.float64(gt[3])
        occ = valid - noc
        bad[0] = _bad(epe, valid, gmag).sum()
        counts[:3] = valid.sum(), noc.sum(), occ.sum()
        errors[:4] = ((epe * valid).sum() / counts[0], (epe * noc).sum() / counts[1], (epe * occ).sum() / max(counts[2], 1.0),
                      bad[0] / counts[0] * 100.0)
        if move is not None:
            mv, st = valid * np.float64(move), valid * (1.0 - np.float64(move))
            bad[1:] = _bad(epe, mv, gmag).sum(), _bad(epe, st, gmag).sum()
            counts[3:] = mv.sum(), st.sum()
            errors[4:] = ((epe * mv).sum() / counts[3], (epe * st).sum() / counts[4], bad[1] / counts[3] * 100.0,
                          bad[2] / counts[4] * 100.0)
    return errors, counts, bad


def bound(gt, pred, f64):
    """The derived bound of a mean or rate of one item: 8 eps32 (max |rescaled pred| + max |gt_uv|) + 4 eps32 |f64| -- the
    four-tap float interpolation and the subtraction lose at most a few ulp of the largest operand per pixel, and a mean
    cannot be further off than its worst pixel; the second term is the rounding of the value itself."""
    big = np.abs(rescale64(pred, gt.shape[-2:])).max() + np.abs(np.float64(gt[:2])).max()
    return 8 * EPS32 * big + 4 * EPS32 * np.abs(f64)


def _vectors(rng, shape, lo, hi, angle=None, spread=np.pi):
    mag = rng.uniform(lo, hi, shape)
    th = (rng.uniform(-np.pi, np.pi) if angle is None else angle) + rng.uniform(-spread, spread, shape)
    return np.stack([mag * np.cos(th), mag * np.sin(th)], axis=-3)


def make_case(name, seed_offset=0):
    """-> dict of float32 arrays: pred [B,2,h,w], gt [B,4,H,W] = (u, v, valid, noc), move [B,H,W].  The 2-channel form of the
    case is gt[:, :2]."""
    (h, w), (H, W) = CASES[name]
    rng = np.random.default_rng(3000 + 17 * list(CASES).index(name) + seed_offset)
    R = _vectors(rng, (B, h, w), 0.0, 40.0)                                  # the rescaled prediction: [B,2,h,w]
    ph, pw = (h + 2) // 3 + 1, (w + 2) // 3 + 1                              # the planted block: the top-left third (+ 1)
    R[:, :, :ph, :pw] = _vectors(rng, (B, ph, pw), 360.0, 400.0, angle=0.7, spread=0.2)
    pred = (R * np.array([w / W, h / H]).reshape(1, 2, 1, 1)).astype(np.float32)
    P = flow_up64(pred, (H, W))
    pmag = np.sqrt((P ** 2).sum(1))
    big = (rng.random((B, H, W)) < 0.5) & ((pmag < 45.0) | (pmag > 350.0))
    emag = np.where(big, rng.uniform(3.5, 12.0, (B, H, W)), rng.uniform(0.1, 2.5, (B, H, W)))
    eth = rng.uniform(-np.pi, np.pi, (B, H, W))
    uv = P + np.stack([emag * np.cos(eth), emag * np.sin(eth)], axis=1)
    valid = (rng.random((B, H, W)) < 0.6).astype(np.float32)
    noc = valid * (rng.random((B, H, W)) < 0.7)
    if name == NOC_IS_VALID[0]:
        noc[NOC_IS_VALID[1]] = valid[NOC_IS_VALID[1]]
    move = (rng.random((B, H, W)) < 0.4).astype(np.float32)
    gt = np.concatenate([uv, valid[:, None], noc[:, None]], axis=1).astype(np.float32)
    case = {"pred": pred, "gt": gt, "move": move}
    check_case(name, case)
    return case


def check_case(name, case):
    """The conditions on the inputs (module docstring).  Raises AssertionError where one does not hold."""
    gt, pred, move = case["gt"], case["pred"], case["move"]
    assert set(np.unique(gt[:, 2:])) <= {0.0, 1.0} and set(np.unique(move)) <= {0.0, 1.0}
    assert (gt[:, 3] <= gt[:, 2]).all(), "noc is a subset of valid"
    if name == NOC_IS_VALID[0]:
        assert np.array_equal(gt[NOC_IS_VALID[1], 2], gt[NOC_IS_VALID[1], 3])
    seen_bad, seen_over = set(), set()
    for b in range(B):
        epe, gmag = _epe_terms(gt[b], pred[b])
        valid = np.float64(gt[b, 2])
        assert valid.mean() >= 0.25, (name, b, valid.mean())
        assert np.abs(epe - 3.0).min() >= 0.5 - 1e-3, (name, b, np.abs(epe - 3.0).min())
        for m in (valid, valid * move[b], valid * (1.0 - move[b])):
            assert m.sum() > 0, (name, b)
            em = epe * m
            assert np.abs(em - 3.0).min() >= 0.05
            over = em > 3
            assert (np.abs(em / gmag - 0.05)[over] >= 0.005).all(), (name, b)
        over = epe * valid > 3
        seen_over |= set(np.unique(over[valid > 0]).tolist())
        seen_bad |= set(np.unique(_bad(epe, valid, gmag)[over]).tolist())
        ratio = (epe / gmag)[over]
        assert ((ratio >= 0.061) | (ratio <= 0.036)).all(), (name, b)
    assert seen_over == {False, True} and seen_bad == {False, True}, (name, seen_over, seen_bad)


def checksums(name, case):
    return {f"{name}_sum_{k}": np.float64(v.astype(np.float64).sum()) for k, v in case.items()}


def form_inputs(case, form, b=None):
    """(gt, pred, move | None) of a form of a case, of the whole batch or of item b."""
    gt = case["gt"][:, :2] if form == "uv" else case["gt"]
    move = case["move"] if form == "move" else None
    if b is None:
        return gt, case["pred"], move
    return gt[b], case["pred"][b], None if move is None else move[b]
