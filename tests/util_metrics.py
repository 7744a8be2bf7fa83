"""Inputs of the depth-metrics fixture (tests/golden/g25_depth_metrics.npz), built the same way by the generator and by the
tests: numpy's frozen default_rng streams, float64 arithmetic rounded once to float32.  The fixture stores a float64 checksum
of every input, so a drift of these streams shows as a failed check, not as a wrong metric.  Also here: the float64 evaluation
of the formulas (source (a) of the fixture; the tests use it for their small hand-made maps too) and the float32 restatement
in the reference's loop order (source (b))."""
import numpy as np

B = 2
# name -> (D, H, W): 36x48 = 1728 pixels, seven workgroups with a partial last one, the wave-layout kernel; 9x12 one partial
# workgroup, odd H; 7x13 = 91 pixels, no multiple of 4: the any-shape kernel; d6: six planes, two of the four plane groups of
# a wave run out of planes after one
CASES = {"36x48": (16, 36, 48), "9x12": (16, 9, 12), "7x13": (16, 7, 13), "d6": (6, 10, 14)}
NAMES = ("mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log", "abs relative",
         "squared relative")


def d_candi(D):
    return [5.0 + (40.0 - 5.0) * v for v in np.linspace(0, 1, D)]   # powerf(5, 40, D, 1)


def make_case(name):
    """-> dict of float32 arrays: logp [B,D,H,W] (a log-softmax), pred [B,H,W] (its expectation, formed in float64 and rounded
    once), truth [B,H,W] (the prediction times a log-normal factor; 0 = no measurement on ~40 % of the pixels; some values beyond
    the last candidate), mask [B,1,H,W] (1 where the truth is there, less a tenth of those)."""
    D, H, W = CASES[name]
    rng = np.random.default_rng(2500 + list(CASES).index(name))
    x = 2.0 * rng.standard_normal((B, D, H, W))
    x = x - x.max(1, keepdims=True)
    logp = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
    dc = np.asarray(d_candi(D), dtype=np.float32).astype(np.float64).reshape(1, D, 1, 1)
    pred = (dc * np.exp(logp.astype(np.float64))).sum(1).astype(np.float32)
    truth = pred.astype(np.float64) * np.exp(0.35 * rng.standard_normal((B, H, W)))
    truth[rng.random((B, H, W)) < 0.4] = 0.0
    mask = ((truth > 0) & (rng.random((B, H, W)) < 0.9)).astype(np.float32)[:, None]
    return {"logp": logp, "pred": pred, "truth": truth.astype(np.float32), "mask": mask}


def checksums(name, inp):
    return {f"{name}_sum_{k}": np.float64(v.astype(np.float64).sum()) for k, v in inp.items()}


def _prepare(pred, truth, mask, clamp_max):
    """The float32 maps that reach depthError: (the masked prediction, the clamped truth with -1 for 0)."""
    p = np.asarray(pred, dtype=np.float32)
    if mask is not None:
        p = (p * np.asarray(mask, dtype=np.float32)).astype(np.float32)
    t = np.array(truth, dtype=np.float32)
    if clamp_max is not None:
        t[t >= np.float32(clamp_max)] = np.float32(clamp_max)
    t[t == 0] = -1.0
    return p, t


def metrics64(pred, truth, mask=None, clamp_max=None):
    """The formulas in float64 on the float32 inputs of one item ([H,W] maps) -> (nine values, n).  n == 0: nine NaNs."""
    p, t = _prepare(pred, truth, mask, clamp_max)
    valid = p > 0
    n = int(valid.sum())
    if n == 0:
        return np.full(9, np.nan), 0
    p, t = p[valid].astype(np.float64), t[valid].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(p - t)
        ei = np.abs(1.0 / p - 1.0 / t)
        s = np.log(p) - np.log(t)
        el = np.abs(s)
        sq_log = (el * el).sum() / n
        out = [e.sum() / n, np.sqrt((e * e).sum() / n), ei.sum() / n, np.sqrt((ei * ei).sum() / n), el.sum() / n, np.sqrt(sq_log),
               np.sqrt(sq_log - s.sum() ** 2 / (float(n) * n)), (e / p).sum() / n, (e * e / (p * p)).sum() / n]
    return np.asarray(out, dtype=np.float64), n


def sil_parts(pred, truth, mask=None, clamp_max=None):
    """(S el^2 / n, (S s)^2 / n^2) in float64: the two terms whose difference the scale-invariant error takes the root of."""
    p, t = _prepare(pred, truth, mask, clamp_max)
    valid = p > 0
    n = int(valid.sum())
    s = np.log(p[valid].astype(np.float64)) - np.log(t[valid].astype(np.float64))
    return (s * s).sum() / n, s.sum() ** 2 / (float(n) * n)


def metrics_seq32(pred, truth, mask=None, clamp_max=None):
    """depthError restated in float32 in its loop order: the column u is the outer loop, the row v the inner one, every
    accumulator a float that takes one pixel at a time; the inverse error is formed in double and rounded (1.0 / x), the rest
    in float -> (nine float32 values, n)."""
    f32 = np.float32
    p, t = _prepare(pred, truth, mask, clamp_max)
    p = p.copy()
    p[p == 0] = -1.0   # (utils/img_utils.py:20; a pixel is valid where this is >= 0)
    H, W = p.shape
    err = [f32(0)] * 9
    log_sum = f32(0)
    n = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for u in range(W):
            for v in range(H):
                gt, ip = p[v, u], t[v, u]
                if not gt >= 0:
                    continue
                d = f32(abs(f32(gt - ip)))
                d2 = f32(d * d)
                di = f32(abs(1.0 / np.float64(gt) - 1.0 / np.float64(ip)))
                dl = f32(abs(f32(np.log(gt) - np.log(ip))))
                err[0] = f32(err[0] + d)
                err[1] = f32(err[1] + d2)
                err[2] = f32(err[2] + di)
                err[3] = f32(err[3] + f32(di * di))
                err[4] = f32(err[4] + dl)
                err[5] = f32(err[5] + f32(dl * dl))
                log_sum = f32(log_sum + f32(np.log(gt) - np.log(ip)))
                err[7] = f32(err[7] + f32(d / gt))
                err[8] = f32(err[8] + f32(d2 / f32(gt * gt)))
                n += 1
        if n == 0:
            return np.full(9, np.nan, dtype=np.float32), 0
        fn = f32(n)
        sq_log = f32(err[5] / fn)
        out = [f32(err[0] / fn), np.sqrt(f32(err[1] / fn)), f32(err[2] / fn), np.sqrt(f32(err[3] / fn)), f32(err[4] / fn),
               np.sqrt(sq_log), np.sqrt(f32(sq_log - f32(f32(log_sum * log_sum) / f32(fn * fn)))), f32(err[7] / fn), f32(err[8] / fn)]
    return np.asarray(out, dtype=np.float32), n
