"""CPU suite of the evaluation metrics: img_utils.eval_errors (plain host code) against hand-made lists and the reference's
evaluateErrors (fixture g25); the C ABI of the depth metrics (pdepth_depth_metrics_workspace_bytes, pdepth_depth_metrics_f32) is
declared, bound and exported, keeps ABI 6 and validates its arguments before any launch (no GPU needed: every call below
returns before touching a pointer); the bindings refuse a CPU tensor; the header says which map is the denominator; the
fixture's inputs are the generators' and its three sources agree."""
import os
import re

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.utils import img_utils
from util import golden
import util_metrics as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdepth_depth_metrics_workspace_bytes", "pdepth_depth_metrics_f32")
FAKE = 256   # a non-null, 256-byte aligned "device pointer": validation fails before any use of it


def test_eval_errors_names_order_and_quirks():
    rows = [[0.5, 2.0, 0.25, 3.0, 0.125, 1.5, 0.75, 4.0, 0.0625], [0.25, 4.0, 0.5, 5.0, 0.375, 2.5, 0.5, 2.0, 0.03125]]
    r = img_utils.eval_errors(rows)
    assert tuple(r) == ops.DEPTH_METRIC_NAMES == U.NAMES
    assert ops.DEPTH_METRIC_NAMES[1] == "rmse" and ops.DEPTH_METRIC_NAMES[6] == "scale invariant log"
    assert r["mae"] == [0.375, 0.25, 0.5]
    assert r["rmse"] == [3.0, 1.0, 4.0]              # every value above 1: the minimum is the 1 it starts from
    assert r["abs relative"] == [3.0, 1.0, 4.0]
    assert r["squared relative"] == [0.046875, 0.03125, 0.0625]
    neg = img_utils.eval_errors([[-1.0] * 9, [-3.0] * 9])
    assert neg["mae"] == [-2.0, -3.0, 0.0]           # every value below 0: the maximum is the 0 it starts from
    assert all(isinstance(v, float) for v in r["mae"])
    # the mean is a float32 accumulation in list order: 1 + 2^-24 + 2^-24 stays 1 in float32, 2^-24 + 2^-24 + 1 does not
    tiny = float(2.0 ** -24)
    assert img_utils.eval_errors([[1.0] * 9, [tiny] * 9, [tiny] * 9])["mae"][0] == float(np.float32(1.0) / np.float32(3.0))
    assert img_utils.eval_errors([[tiny] * 9, [tiny] * 9, [1.0] * 9])["mae"][0] == float(np.float32(1.0 + 2.0 ** -23) / np.float32(3.0))
    nan = img_utils.eval_errors([[float("nan")] * 9, [0.5] * 9])
    assert np.isnan(nan["mae"][0]) and nan["mae"][1:] == [0.5, 0.5]
    with pytest.raises(RuntimeError):
        img_utils.eval_errors([])


def test_eval_errors_against_the_reference():
    g = golden("g25_depth_metrics.npz")
    assert int(g["has_ref"]) == 1
    rows = [g[name + "_ref"][b].tolist() for name in U.CASES for b in range(U.B)]
    r = img_utils.eval_errors(rows)
    for i, name in enumerate(ops.DEPTH_METRIC_NAMES):
        assert np.array_equal(np.asarray(r[name], dtype=np.float32), g["ee_ref"][i]), name


def test_fixture_inputs_and_sources():
    g = golden("g25_depth_metrics.npz")
    for name in U.CASES:
        for k, v in U.checksums(name, U.make_case(name)).items():
            assert g[k] == v, k
        a = g[name + "_f64"]
        for other in ("_seq32", "_ref"):
            assert np.all(np.abs(g[name + other] - a) <= 1e-4 * np.abs(a)), (name, other)
        assert g[name + "_n"].shape == (U.B,) and np.isfinite(a).all() and (a > 0).all()
    inp = U.make_case("9x12")
    a, n = U.metrics64(inp["pred"][1], inp["truth"][1], inp["mask"][1, 0], U.d_candi(16)[-1])
    assert n == g["9x12_n"][1] and np.array_equal(a, g["9x12_f64"][1])
    s, _ = U.metrics_seq32(inp["pred"][1], inp["truth"][1], inp["mask"][1, 0], U.d_candi(16)[-1])
    assert np.array_equal(s, g["9x12_seq32"][1])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g25_depth_metrics.npz")) < 32 * 1024


def test_new_symbols_declared_bound_exported_abi_unchanged():
    lib = _native.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pdepth.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pdepth_[a-z0-9_]+)\s*\(", text))
    for sym in NEW:
        assert sym in declared and sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6
    h = open(os.path.join(REPO, "include", "pdepth.h")).read()
    assert "#define PDEPTH_ABI_VERSION 6" in h
    additions = h[h.index("backward-compatible additions within 6"):h.index("enum", h.index("backward-compatible additions within 6"))]
    for sym in NEW:
        assert sym in additions, sym


def _call(logp=None, pred=FAKE, dc=None, truth=FAKE * 2, mask=None, clamp=40.0, B=1, D=0, H=2, W=2, metrics=FAKE * 3, count=FAKE * 4,
          depth=None, ws=FAKE * 5, ws_bytes=None):
    import ctypes
    lib = _native.load()
    if ws_bytes is None:
        ws_bytes = lib.pdepth_depth_metrics_workspace_bytes(max(B, 1), max(H, 1), max(W, 1))
    rc = lib.pdepth_depth_metrics_f32(logp, pred, dc, truth, mask, ctypes.c_float(clamp), B, D, H, W, metrics, count, depth, ws, ws_bytes, None)
    return rc, lib.pdepth_last_error().decode()


def test_entry_validation():
    rc, msg = _call(truth=None)
    assert rc == 1 and "pdepth_depth_metrics_f32: null pointer" in msg
    rc, msg = _call(logp=FAKE * 6, dc=FAKE * 7, D=4)             # both predictions
    assert rc == 1 and "exactly one prediction" in msg
    rc, msg = _call(pred=None)                                   # neither
    assert rc == 1 and "exactly one prediction" in msg
    rc, msg = _call(pred=None, logp=FAKE * 6, dc=None, D=4)      # a volume without its candidates
    assert rc == 1 and "d_candi" in msg
    for dims in (dict(B=0), dict(H=-1), dict(W=0)):
        rc, msg = _call(**dims)
        assert rc == 1 and "non-positive dimension" in msg, dims
    rc, msg = _call(pred=None, logp=FAKE * 6, dc=FAKE * 7, D=0)
    assert rc == 1 and "non-positive dimension" in msg
    rc, msg = _call(metrics=None)
    assert rc == 1 and "null output pointer" in msg
    rc, msg = _call(depth=FAKE * 8)                              # the depth map form is given its map
    assert rc == 1 and "volume form" in msg
    lib = _native.load()
    need = lib.pdepth_depth_metrics_workspace_bytes(2, 36, 48)
    assert need >= 2 * 7 * 80 and need % 256 == 0                # seven workgroups per item, nine sums and the count each
    for dims in ((0, 36, 48), (2, 0, 48), (2, 36, -1)):
        assert lib.pdepth_depth_metrics_workspace_bytes(*dims) == 0, dims
    rc, msg = _call(B=2, H=36, W=48, ws_bytes=need - 1)
    assert rc == 3 and "workspace" in msg
    rc, msg = _call(B=2, H=36, W=48, ws=None, ws_bytes=need)
    assert rc == 3
    rc, msg = _call(B=2, H=36, W=48, ws=FAKE * 5 + 8, ws_bytes=need)
    assert rc == 3 and "aligned" in msg


def test_bindings_refuse_before_the_device():
    truth, pred = torch.ones(1, 4, 4), torch.ones(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics(truth, pred=pred)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_metrics(truth, logp=torch.zeros(1, 6, 4, 4), d_candi=[1.0] * 6)
    with pytest.raises(RuntimeError, match="exactly one prediction"):
        ops.depth_metrics(truth)
    with pytest.raises(RuntimeError, match="exactly one prediction"):
        ops.depth_metrics(truth, pred=pred, logp=torch.zeros(1, 6, 4, 4), d_candi=[1.0] * 6)
    with pytest.raises(RuntimeError, match=r"pred must be \[1, 4, 4\]"):
        ops.depth_metrics(truth, pred=torch.ones(1, 4, 5))
    with pytest.raises(RuntimeError, match="d_candi has 8 entries, volume has D=6"):
        ops.depth_metrics(truth, logp=torch.zeros(1, 6, 4, 4), d_candi=[1.0] * 8)
    with pytest.raises(RuntimeError, match="want_depth"):
        ops.depth_metrics(truth, pred=pred, want_depth=True)
    with pytest.raises(RuntimeError, match="no backward"):
        ops.depth_metrics(truth, pred=pred.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        img_utils.depth_error(torch.ones(4, 4), torch.ones(4, 4))


def test_header_and_docstrings_name_the_denominator():
    h = open(os.path.join(REPO, "include", "pdepth.h")).read()
    prose = h[h.index("Evaluation metrics: the KITTI devkit"):h.index("size_t pdepth_depth_metrics_workspace_bytes")]
    assert "prediction as denominator" in prose and "depthError(D_gt, D_ipol)" in prose
    assert "abs relative = S (e / p) / n" in prose and "count[b] = 0" in prose
    for doc in (ops.depth_metrics.__doc__, img_utils.depth_error.__doc__):
        assert "depthError(D_gt, D_ipol)" in doc and "divide" in doc
    import pdepth_amd.harness as harness
    assert "out of scope" not in harness.__doc__.split("Dataset IO")[0] and callable(harness.validate) and callable(harness.validate_step)
