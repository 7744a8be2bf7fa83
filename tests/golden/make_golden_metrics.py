"""Golden fixture g25: the KITTI devkit's nine depth errors.  Build container only (reads the reference, which never travels):

    python tests/golden/make_golden_metrics.py

Inputs: tests/util_metrics.py (B = 2; 36 x 48, 9 x 12 and 7 x 13 at D = 16, 10 x 14 at D = 6; rebuilt by the tests from the same
frozen random streams -- the fixture stores their checksums).  Every item is evaluated as the evaluation loop does
(trainer/default_trainer.py:247-256: the truth clamped at the last candidate, the prediction times the mask).  Stored per case,
from three sources:
  (a) `<case>_f64`, `<case>_n`: a float64 evaluation of the formulas (util_metrics.metrics64);
  (b) `<case>_seq32`: a float32 restatement of depthError in its loop order (util_metrics.metrics_seq32);
  (c) `<case>_ref`: the reference's own depthError (external/deval_lib/src/evaluate_depth.h:20-121), called with the arguments
      in img_utils.depth_error's order, and `ee_ref`, its evaluateErrors over all items of the fixture in case order.
For (c) the devkit's headers are compiled with g++ in a temporary directory outside the repository, behind a small
extern "C" shim called through ctypes; libpng and png++ are not installed here, so a stand-in png++/png.hpp (written by this
script: an image class that holds pixels in memory and a reader that reads nothing) satisfies the headers' include --
depthError touches DepthImage's pointer constructor, width, height, isValid and getDepth only.  Nothing of the reference, or
compiled from it, is kept: the directory is removed, the fixture holds numbers only.
Asserted here, because the tests' tolerances rest on it: every item has S el^2 / n - (S s)^2 / n^2 >= 0.05 S el^2 / n (the
scale-invariant error is well conditioned) and at least 25 % valid pixels; (b) and (c) agree with (a) to 1e-4 relative; the
clamp, the mask and the zero truth are all exercised.
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import util_metrics as U  # noqa: E402

DEVKIT = "/root/reference/external/deval_lib/src"

PNG_STAND_IN = r"""
#pragma once
#include <cstddef>
#include <cstdint>
#include <istream>
#include <string>
#include <vector>
namespace png {
typedef uint16_t gray_pixel_16;
struct rgb_pixel {
  uint8_t red, green, blue;
  rgb_pixel() : red(0), green(0), blue(0) {}
  rgb_pixel(uint8_t r, uint8_t g, uint8_t b) : red(r), green(g), blue(b) {}
};
enum color_type { color_type_gray = 0 };
template <class P> class image {
 public:
  image(size_t w = 0, size_t h = 0) : w_(w), h_(h), d_(w * h) {}
  explicit image(const std::string&) : w_(0), h_(0) {}
  size_t get_width() const { return w_; }
  size_t get_height() const { return h_; }
  P get_pixel(size_t u, size_t v) const { return d_[v * w_ + u]; }
  void set_pixel(size_t u, size_t v, P p) { d_[v * w_ + u] = p; }
  void write(const std::string&) {}
 private:
  size_t w_, h_;
  std::vector<P> d_;
};
template <class S> class reader {
 public:
  explicit reader(S&) {}
  void read_info() {}
  color_type get_color_type() const { return color_type_gray; }
  size_t get_bit_depth() const { return 16; }
  size_t get_width() const { return 0; }
  size_t get_height() const { return 0; }
};
}  // namespace png
"""

SHIM = r"""
#include <algorithm>
#include "evaluate_depth.h"
static const char* kNames[9] = {"mae", "rmse", "inverse mae", "inverse rmse", "log mae", "log rmse", "scale invariant log",
                                "abs relative", "squared relative"};
extern "C" int shim_depth_error(const float* first, const float* second, int w, int h, float* out) {
  try {
    DepthImage a(first, w, h), b(second, w, h);
    std::vector<float> e = depthError(a, b);
    for (int i = 0; i < 9; i++) out[i] = e[i];
    return 0;
  } catch (...) {
    return 1;
  }
}
extern "C" void shim_evaluate_errors(const float* rows, int n, float* out) {
  std::vector<std::vector<float>> errs;
  for (int i = 0; i < n; i++) errs.push_back(std::vector<float>(rows + 9 * i, rows + 9 * i + 9));
  std::map<std::string, std::vector<float>> r = evaluateErrors(errs);
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 3; j++) out[3 * i + j] = r[kNames[i]][j];
}
"""


def build_reference():
    """-> (ctypes library of the devkit's depthError / evaluateErrors, its temporary directory) or (None, None)."""
    if not os.path.isdir(DEVKIT) or shutil.which("g++") is None:
        return None, None
    tmp = tempfile.mkdtemp(prefix="g25_devkit_")
    os.makedirs(os.path.join(tmp, "png++"))
    with open(os.path.join(tmp, "png++", "png.hpp"), "w") as f:
        f.write(PNG_STAND_IN)
    with open(os.path.join(tmp, "shim.cpp"), "w") as f:
        f.write(SHIM)
    so = os.path.join(tmp, "libshim.so")
    r = subprocess.run(["g++", "-O2", "-w", "-shared", "-fPIC", "-I", tmp, "-I", DEVKIT, os.path.join(tmp, "shim.cpp"), "-o", so],
                       capture_output=True, text=True)
    if r.returncode != 0:
        print("the devkit did not compile behind the stand-in:\n" + r.stderr[-3000:])
        shutil.rmtree(tmp)
        return None, None
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.shim_depth_error.argtypes = [fp, fp, ctypes.c_int, ctypes.c_int, fp]
    lib.shim_depth_error.restype = ctypes.c_int
    lib.shim_evaluate_errors.argtypes = [fp, ctypes.c_int, fp]
    return lib, tmp


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def reference_depth_error(lib, predicted, truth):
    """utils/img_utils.py:17-22: zeros to -1, `+ epsilon` (a float32 no-op), then depthError(predicted, truth)."""
    eps = np.finfo(float).eps
    p, t = predicted.copy(), truth.copy()
    p[p == 0] = -1
    t[t == 0] = -1
    p, t = np.ascontiguousarray(p + eps, dtype=np.float32), np.ascontiguousarray(t + eps, dtype=np.float32)
    out = np.zeros(9, dtype=np.float32)
    rc = lib.shim_depth_error(_fp(p), _fp(t), p.shape[1], p.shape[0], _fp(out))
    return out if rc == 0 else None


def main():
    lib, tmp = build_reference()
    out = {"has_ref": np.int32(lib is not None)}
    rows_ref = []
    try:
        for name, (D, H, W) in U.CASES.items():
            inp = U.make_case(name)
            out.update(U.checksums(name, inp))
            clamp = U.d_candi(D)[-1]
            f64, seq, ref, ns = [], [], [], []
            for b in range(U.B):
                args = (inp["pred"][b], inp["truth"][b], inp["mask"][b, 0], clamp)
                a, n = U.metrics64(*args)
                s32, n32 = U.metrics_seq32(*args)
                assert n == n32 and n >= 0.25 * H * W, (name, b, n)
                sq, mean_sq = U.sil_parts(*args)
                assert sq - mean_sq >= 0.05 * sq, (name, b, sq, mean_sq)
                assert np.all(np.abs(s32 - a) <= 1e-4 * np.abs(a)), (name, b, s32, a)
                assert (inp["truth"][b] >= clamp).any() and (inp["truth"][b] == 0).any(), (name, b)
                assert ((inp["mask"][b, 0] == 0) & (inp["truth"][b] > 0)).any(), (name, b)
                f64.append(a), seq.append(s32), ns.append(n)
                if lib is not None:
                    p, t = U._prepare(*args)
                    t[t == -1] = 0   # (the trainer's maps: _prepare has already made the reference's 0 -> -1 step)
                    r = reference_depth_error(lib, p, t)
                    assert r is not None and np.all(np.abs(r - a) <= 1e-4 * np.abs(a)), (name, b, r, a)
                    ref.append(r), rows_ref.append(r)
                    print(name, b, "n", n, "max |seq32 - f64| / f64", float(np.max(np.abs(s32 - a) / a)),
                          "max |ref - f64| / f64", float(np.max(np.abs(r - a) / a)), "ref == seq32:", bool(np.array_equal(r, s32)))
            out[name + "_f64"], out[name + "_seq32"], out[name + "_n"] = np.stack(f64), np.stack(seq), np.asarray(ns, dtype=np.int64)
            if lib is not None:
                out[name + "_ref"] = np.stack(ref)
        if lib is not None:
            # no valid pixel: the reference throws
            assert reference_depth_error(lib, np.zeros((3, 4), np.float32), np.ones((3, 4), np.float32)) is None
            rows = np.ascontiguousarray(np.stack(rows_ref), dtype=np.float32)
            ee = np.zeros(27, dtype=np.float32)
            lib.shim_evaluate_errors(_fp(rows), rows.shape[0], _fp(ee))
            out["ee_ref"] = ee.reshape(9, 3)
    finally:
        if tmp is not None:
            del lib
            shutil.rmtree(tmp)
    path = os.path.join(HERE, "g25_depth_metrics.npz")
    np.savez_compressed(path, **out)
    print("reference values stored:", bool(out["has_ref"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
