"""CPU suite of the flow evaluation: the float64 statement (util_flow_metrics.metrics64) against the fixture g30 and the
reference's own float32 values in it; the inputs' conditions; the C ABI of csrc/flow_metrics.hip is declared, bound and exported,
keeps ABI 6 and validates its arguments before any launch (no GPU needed: every call below returns before touching a pointer);
the bindings refuse a CPU tensor."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, harness, ops
from pdepth_amd.utils import flow_utils
from util import golden
import util_flow_metrics as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pdepth_flow_metrics_workspace_bytes", "pdepth_flow_metrics_f32", "pdepth_flow_resize_f32")
FAKE = 256   # a non-null, 256-byte aligned "device pointer": validation fails before any use of it


@pytest.mark.parametrize("name", list(U.CASES))
def test_metrics64_against_the_fixture(name):
    g = golden("g30_flow_metrics.npz")
    case = U.make_case(name)                       # (asserts the conditions on the inputs)
    for k, v in U.checksums(name, case).items():
        assert g[k] == v, k
    for form in U.FORMS:
        key = f"{name}_{form}"
        n = {"uv": 1, "masks": 4, "move": 6}[form]
        for b in range(U.B):
            gt, pred, move = U.form_inputs(case, form, b)
            errors, counts, bad = U.metrics64(gt, pred, move)
            assert np.array_equal(errors, g[key + "_f64"][b], equal_nan=True), key
            assert np.array_equal(counts, g[key + "_counts"][b], equal_nan=True) and np.array_equal(bad, g[key + "_bad"][b]), key
            # the reference's float32 run: the values it returns, a float32's rounding of the sums away from the float64 ones
            ref32 = np.float64(g[key + "_ref32"][b])
            assert np.isfinite(ref32[:n]).all() and np.isnan(ref32[n:]).all()
            assert (np.abs(ref32[:n] - errors[:n]) <= 1e-4 * np.maximum(np.abs(errors[:n]), 1.0)).all(), (key, ref32, errors)
    if name == U.NOC_IS_VALID[0]:
        f = g[f"{name}_masks_f64"][U.NOC_IS_VALID[1]]
        assert f[2] == 0.0 and g[f"{name}_masks_counts"][U.NOC_IS_VALID[1]][2] == 0.0       # the max(., 1) branch
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g30_flow_metrics.npz")) < 64 * 1024


def test_resize64_is_interpolate_in_exact_arithmetic():
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    for (h, w), (H, W) in list(U.CASES.values())[:6]:
        x = rng.standard_normal((2, 2, h, w))
        for ac in (False, True):
            want = F.interpolate(torch.from_numpy(x), size=(H, W), mode="bilinear", align_corners=ac).numpy()
            assert np.abs(U.resize64(x, (H, W), ac) - want).max() <= 1e-13, ((h, w), (H, W), ac)


def test_new_symbols_declared_bound_exported_abi_unchanged():
    lib = _native.load()
    h = open(os.path.join(REPO, "include", "pdepth.h")).read()
    declared = set(re.findall(r"\b(pdepth_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S)))
    additions = h[h.index("backward-compatible additions within 6"):h.index("enum", h.index("backward-compatible additions within 6"))]
    for sym in NEW:
        assert sym in declared and sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym in additions, sym
        assert sym in _native._ABSENT_FROM_EXPERIMENT_LIBS
        assert next(src for part, src in _native._SOURCE_OF_ENTRY.items() if part in sym) == "csrc/flow_metrics.hip"
    assert next(src for part, src in _native._SOURCE_OF_ENTRY.items() if part in "pdepth_flow_warp_f32") == "csrc/flow_warp.hip"
    assert lib.pdepth_abi_version() == 6 and "#define PDEPTH_ABI_VERSION 6" in h
    mk = open(os.path.join(REPO, "probabilistic-depth_amd", "csrc", "Makefile")).read()
    assert "flow_metrics.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert ops.FLOW_METRIC_NAMES == U.NAMES and callable(harness.validate_flow)
    assert "out of scope" in flow_utils.__doc__.lower() and "in place" in flow_utils.resize_flow.__doc__


def _metrics(gt=FAKE, ch=4, pred=FAKE * 2, h=3, w=4, move=None, B=2, H=36, W=48, errors=FAKE * 3, counts=FAKE * 4, flow_up=None,
             ws=FAKE * 5, ws_bytes=None):
    lib = _native.load()
    if ws_bytes is None:
        ws_bytes = lib.pdepth_flow_metrics_workspace_bytes(max(B, 1), max(H, 1), max(W, 1))
    rc = lib.pdepth_flow_metrics_f32(gt, ch, pred, h, w, move, B, H, W, errors, counts, flow_up, ws, ws_bytes, None)
    return rc, lib.pdepth_last_error().decode()


def test_entry_validation():
    lib = _native.load()
    for kw in (dict(gt=None), dict(pred=None)):
        rc, msg = _metrics(**kw)
        assert rc == 1 and "pdepth_flow_metrics_f32: null pointer" in msg, kw
    for ch in (3, 0, 1, 5):
        rc, msg = _metrics(ch=ch)
        assert rc == 1 and f"gt_channels={ch}" in msg
    rc, msg = _metrics(ch=2, move=FAKE * 6)
    assert rc == 1 and "move mask needs a truth of 4 channels" in msg
    for dims in (dict(B=0), dict(H=-1), dict(W=0), dict(h=0), dict(w=-3)):
        rc, msg = _metrics(**dims)
        assert rc == 1 and "non-positive dimension" in msg, dims
    rc, msg = _metrics(B=65536)
    assert rc == 1 and "at most 65535" in msg
    rc, msg = _metrics(h=1 << 16, w=1 << 15)
    assert rc == 1 and "2^30" in msg
    for kw in (dict(errors=None), dict(counts=None)):
        rc, msg = _metrics(**kw)
        assert rc == 1 and "null output pointer" in msg
    need = lib.pdepth_flow_metrics_workspace_bytes(2, 36, 48)
    assert need >= 2 * 7 * 104 and need % 256 == 0               # seven workgroups per item, thirteen sums each
    for dims in ((0, 36, 48), (2, 0, 48), (2, 36, -1), (1, 1 << 16, 1 << 15)):
        assert lib.pdepth_flow_metrics_workspace_bytes(*dims) == 0, dims
    rc, msg = _metrics(ws_bytes=need - 1)
    assert rc == 3 and "workspace" in msg
    rc, msg = _metrics(ws=None, ws_bytes=need)
    assert rc == 3
    rc, msg = _metrics(ws=FAKE * 5 + 8, ws_bytes=need)
    assert rc == 3 and "aligned" in msg
    rc, msg = _metrics(ch=3, ws=None, ws_bytes=0)                # the arguments before the workspace
    assert rc == 1
    # the resize
    rs = lib.pdepth_flow_resize_f32
    said = lambda rc, code, text: rc == code and text in lib.pdepth_last_error().decode()   # noqa: E731
    assert said(rs(None, 2, 3, 4, 6, 8, 0, FAKE, None), 1, "pdepth_flow_resize_f32: null pointer")
    assert said(rs(FAKE, 2, 3, 4, 6, 8, 0, None, None), 1, "null output pointer")
    assert said(rs(FAKE, 2, 3, 4, 6, 8, 0, FAKE, None), 1, "alias")
    assert said(rs(FAKE, 2, 3, 4, 6, 8, 2, FAKE * 2, None), 1, "align_corners=2")
    assert said(rs(FAKE, 2, 0, 4, 6, 8, 0, FAKE * 2, None), 1, "non-positive dimension")
    assert said(rs(FAKE, 2, 3, 4, 6, -8, 1, FAKE * 2, None), 1, "non-positive dimension")
    assert said(rs(FAKE, 2, 3, 4, 1 << 16, 1 << 15, 1, FAKE * 2, None), 1, "2^30")


def test_bindings_refuse_before_the_device():
    gt, pred = torch.zeros(1, 4, 4, 6), torch.zeros(1, 2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_metrics(gt, pred)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_metrics(gt[:, :2], pred, want_flow=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_resize(pred, (4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_utils.resize_flow(pred, (4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_utils.evaluate_flow(gt, pred)
    with pytest.raises(RuntimeError, match=r"gt must be \[B,2,H,W\] or \[B,4,H,W\]"):
        ops.flow_metrics(torch.zeros(1, 3, 4, 6), pred)
    with pytest.raises(RuntimeError, match=r"pred must be \[1, 2, h, w\]"):
        ops.flow_metrics(gt, torch.zeros(2, 2, 2, 3))
    with pytest.raises(RuntimeError, match="move mask needs a truth of 4 channels"):
        ops.flow_metrics(gt[:, :2], pred, move_mask=torch.zeros(1, 4, 6))
    with pytest.raises(RuntimeError, match=r"move_mask must be \[1, 4, 6\]"):
        ops.flow_metrics(gt, pred, move_mask=torch.zeros(1, 4, 5))
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.flow_metrics(gt, pred.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.flow_resize(pred.clone().requires_grad_(True), (4, 6))
    with pytest.raises(RuntimeError, match=r"flow must be \[B,2,h,w\]"):
        ops.flow_resize(torch.zeros(1, 3, 2, 3), (4, 6))
