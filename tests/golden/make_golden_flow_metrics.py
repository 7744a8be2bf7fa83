"""Golden fixture g30: the flow evaluation.  Build container only (reads the reference, which never travels):

    python tests/golden/make_golden_flow_metrics.py [path of the reference tree]

Per case and form (tests/util_flow_metrics.py: CASES x FORMS; the inputs are regenerated from seeds, not stored) it runs the
reference's own utils/flow_utils.evaluate_flow, one item at a time, on the float32 inputs, and stores
  <case>_<form>_ref32  [B,6]  what it returns (1, 4 or 6 values; the rest NaN), in float32 arithmetic as the trainers call it;
  <case>_<form>_f64    [B,8]  metrics64, the float64 statement of the formulas (errors);
  <case>_<form>_counts [B,5]  the mask sums;  <case>_<form>_bad [B,3]  the three bad-pixel counts (-1: not defined);
and a float64 checksum of every input.

OpenCV is not installed where this runs.  Before the reference is imported a stand-in module named `cv2` is put into
sys.modules, with INTER_LINEAR and resize(src, (W, H), interpolation=) only.  That resize is written here, in numpy, from
OpenCV's documented rule for INTER_LINEAR: half-pixel centres, fx = (dx + 0.5) * (w / W) - 0.5 formed in double and rounded to
the element type, sx = floor(fx), fx -= sx; sx < 0 -> (0, fx = 0); sx >= w - 1 -> (w - 1, fx = 0); the weights 1 - fx and fx in
the element type; the two rows are interpolated first, then the column; no antialiasing.  Everything downstream of the resize
-- the rescale, the end-point error, the masked means, the outlier rate -- is the reference's code.  (matplotlib, which the
reference's module imports for flow_to_image, gets an empty stand-in when it is missing.)

The generator also runs the reference on float64 copies of the inputs (the stand-in resizes in the element type of its
argument) and asserts that metrics64 agrees with it to 1e-10: the float64 statement is the reference's formula."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import util_flow_metrics as U  # noqa: E402


def _cv2_resize(src, dsize, interpolation=1):
    assert interpolation == 1
    W, H = dsize
    h, w = src.shape[:2]
    t = src.dtype.type

    def axis(n_out, n_in):
        f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(t)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(t)).astype(t)
        f[s < 0] = 0
        s[s < 0] = 0
        f[s >= n_in - 1] = 0
        s[s >= n_in - 1] = n_in - 1
        return s, np.minimum(s + 1, n_in - 1), f

    (y0, y1, fy), (x0, x1, fx) = axis(H, h), axis(W, w)
    fx, fy = fx.reshape(1, W, 1), fy.reshape(H, 1, 1)
    one = t(1)
    rows = (src[:, x0] * (one - fx) + src[:, x1] * fx).astype(t)      # [h, W, C]: the horizontal pass of every source row
    return (rows[y0] * (one - fy) + rows[y1] * fy).astype(t)


def load_reference(root):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR = 1
    cv2.resize = _cv2_resize
    sys.modules["cv2"] = cv2
    try:
        import matplotlib.colors  # noqa: F401
    except ImportError:
        mpl, colors = types.ModuleType("matplotlib"), types.ModuleType("matplotlib.colors")
        colors.hsv_to_rgb = None
        mpl.colors = colors
        sys.modules["matplotlib"], sys.modules["matplotlib.colors"] = mpl, colors
    spec = importlib.util.spec_from_file_location("reference_flow_utils", os.path.join(root, "utils", "flow_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_item(ref, gt, pred, move, dtype):
    hwc = lambda a: np.ascontiguousarray(np.moveaxis(a, 0, -1).astype(dtype))   # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        return ref.evaluate_flow([hwc(gt)], [hwc(pred)], None if move is None else [move.astype(dtype)])


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
    out = {}
    worst = 0.0
    for name in U.CASES:
        case = U.make_case(name)
        out.update(U.checksums(name, case))
        for form in U.FORMS:
            ref32, f64 = np.full((U.B, 6), np.nan, np.float32), np.zeros((U.B, 8))
            counts, bad = np.zeros((U.B, 5)), np.zeros((U.B, 3))
            for b in range(U.B):
                gt, pred, move = U.form_inputs(case, form, b)
                f64[b], counts[b], bad[b] = U.metrics64(gt, pred, move)
                r32 = reference_item(ref, gt, pred, move, np.float32)
                r64 = reference_item(ref, gt, pred, move, np.float64)
                n = {"uv": 1, "masks": 4, "move": 6}[form]
                assert len(r32) == len(r64) == n
                ref32[b, :n] = r32
                d = np.abs(np.asarray(r64) - f64[b, :n])
                assert (d <= 1e-10 * np.maximum(1.0, np.abs(f64[b, :n]))).all(), (name, form, b, r64, f64[b])
                worst = max(worst, float(d.max()))
            key = f"{name}_{form}"
            out[key + "_ref32"], out[key + "_f64"], out[key + "_counts"], out[key + "_bad"] = ref32, f64, counts, bad
    path = os.path.join(HERE, "g30_flow_metrics.npz")
    np.savez_compressed(path, **out)
    print("max |reference in float64 - metrics64| =", worst, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
