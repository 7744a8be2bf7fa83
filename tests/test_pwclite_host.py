"""CPU suite: models.pwclite.PWCLite against the fixture of the reference's run (tests/golden/g29_pwclite.npz, made by
tests/golden/make_golden_pwclite.py): state-dict names and shapes, parameter counts, the flows of every case at every level against
float64 (on CPU tensors the model is the reference's torch arithmetic), silence, and the refused channel counts."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import util_cost_volume as U
import util_flow as UF
from pdepth_amd import _native, synth
from pdepth_amd.models.pwclite import PWCLite


def _state(model):
    return ["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in model.state_dict().items()]


def _model(frames, reduce_dense, **kw):
    model = PWCLite(U.pwc_cfg(frames, reduce_dense), **kw)
    synth.seed_weights(model, seed=U.PWC_SEED, gain=U.PWC_GAIN)
    return model


@pytest.mark.parametrize("key, frames, reduce_dense", [("state.reduce", 2, True), ("state.dense", 2, False), ("state.reduce3", 3, True)])
def test_state_dict_names_and_shapes_are_the_references(key, frames, reduce_dense):
    want = [str(s) for s in U.fixture()[key]]
    got = _state(PWCLite(U.pwc_cfg(frames, reduce_dense)))
    assert got == want
    for group in ("feature_pyramid_extractor.convs.", "flow_estimators.", "context_networks.convs.", "conv_1x1."):
        assert any(k.startswith(group) for k in got), group


@pytest.mark.parametrize("frames, reduce_dense", sorted(U.PWC_PARAMETERS))
def test_num_parameters(frames, reduce_dense):
    assert PWCLite(U.pwc_cfg(frames, reduce_dense)).num_parameters() == U.PWC_PARAMETERS[(frames, reduce_dense)]


@pytest.mark.parametrize("name", list(U.PWC_CASES))
def test_cpu_flows_against_float64_and_silence(name):
    frames, reduce_dense, with_bk, _ = U.PWC_CASES[name]
    fx = U.fixture()
    model = _model(frames, reduce_dense)
    shown = io.StringIO()
    with torch.no_grad(), contextlib.redirect_stdout(shown):
        flows = U.pwc_flows(model(U.pwc_input(name), with_bk=with_bk))
    assert shown.getvalue() == ""
    assert len(flows) == len([k for k in fx if k.startswith(name + ".") and k.endswith(".v64")])
    for key, f in flows:
        ref = fx[f"{name}.{key}.v64"]
        err = float(np.abs(U.pwc_subset(f.double().numpy()) - ref).max())
        tol = UF.tol(fx[f"{name}.{key}.err"], fx[f"{name}.{key}.max"])
        print(f"{name} {key}: |flow - float64| {err:.2e}, tolerance {tol:.2e}")
        assert err <= tol, (name, key, err, tol)


def test_init_weights_and_frame_counts():
    model = PWCLite(U.pwc_cfg(2, True))
    model.init_weights()
    assert all(float(m.bias.detach().abs().max()) == 0 for m in model.modules() if isinstance(m, torch.nn.Conv2d))
    # off by default: the whole-model measurement of DESIGN.md 6.12 decides it
    assert model.fused_cost is False and PWCLite(U.pwc_cfg(2, True), fused_cost=True).fused_cost is True
    for channels in (3, 7, 12, 18):
        with pytest.raises(NotImplementedError):
            model(torch.zeros(1, channels, 64, 64))


def test_cost_volume_entries_refuse_before_any_launch():
    """The validation paths of the C entries, with code and message; no GPU is touched (the pointers are never read)."""
    lib = _native.load()
    fwd, bwd, det = lib.pdepth_flow_cost_volume_f32, lib.pdepth_flow_cost_volume_backward_f32, lib.pdepth_flow_cost_volume_backward_det_f32
    q, qd = lib.pdepth_flow_cost_volume_backward_workspace_bytes, lib.pdepth_flow_cost_volume_backward_det_workspace_bytes

    def said(rc, code, words):
        return rc == code and words in lib.pdepth_last_error()

    f = ctypes.c_float
    assert said(fwd(None, 512, 768, 2, 3, 8, 8, 4, f(0.1), 0, 1024, None), 1, b"null pointer")
    for md in (0, 5, -1):
        assert said(fwd(256, 512, 768, 2, 3, 8, 8, md, f(0.1), 0, 1024, None), 1, b"max_displacement must be 1..4")
    for slope in (float("nan"), -0.1):
        assert said(fwd(256, 512, 768, 2, 3, 8, 8, 4, f(slope), 0, 1024, None), 1, b"negative_slope is NaN or negative")
    assert said(fwd(256, 512, 768, 2, 3, 8, 8, 4, f(0.1), 2, 1024, None), 1, b"unknown pad")
    assert said(fwd(256, 512, None, 2, 3, 8, 8, 4, f(0.1), 7, 1024, None), 1, b"unknown pad")
    assert said(fwd(256, 512, 768, 2, 3, 1, 8, 4, f(0.1), 0, 1024, None), 1, b"H and W must be at least 2 with a flow")
    assert said(fwd(256, 512, 768, 2, 3, 8, 1, 4, f(0.1), 0, 1024, None), 1, b"H and W must be at least 2 with a flow")
    assert said(fwd(256, 512, None, 2, 3, 0, 8, 4, f(0.1), 0, 1024, None), 1, b"non-positive dimension")
    assert said(fwd(256, 512, 768, 8192, 64, 8, 8, 4, f(0.1), 0, 1024, None), 1, b"B * ceil(C / 8) at most 65535")
    n = 2 * 3 * 8 * 8 * 4
    assert q(2, 3, 8, 8, 1) == n and q(2, 3, 8, 8, 0) == 0 and q(2, 3, 1, 8, 1) == 0 and q(0, 3, 8, 8, 1) == 0
    assert qd(2, 3, 8, 8, 1) == n + lib.pdepth_flow_warp_backward_det_workspace_bytes(2, 3, 8, 8) and qd(2, 3, 8, 8, 0) == 0
    for fn, need in ((bwd, q(2, 3, 8, 8, 1)), (det, qd(2, 3, 8, 8, 1))):
        head = (256, 512, 768, 1024, 1280, 2, 3, 8, 8, 4, f(0.1), 0)
        assert said(fn(*head, None, None, None, 4096, need, None), 1, b"no gradient requested")
        assert said(fn(256, 512, None, 1024, 1280, 2, 3, 8, 8, 4, f(0.1), 0, None, None, 1536, 4096, need, None), 1, b"grad_flow requested without a flow")
        assert said(fn(256, 512, 768, None, 1280, 2, 3, 8, 8, 4, f(0.1), 0, 1536, None, None, 4096, need, None), 1, b"null pointer")
        assert said(fn(*head, 1536, 1792, None, None, 0, None), 3, b"bytes of workspace (got 0); query pdepth_flow_cost_volume_backward")
        assert said(fn(*head, 1536, 1792, None, 4096, need - 1, None), 3, b"bytes of workspace")
        assert said(fn(*head, 1536, 1792, None, 4096 + 64, need, None), 3, b"256-byte aligned")
        assert said(fn(256, 512, 768, 1024, 1280, 2, 3, 8, 8, 5, f(0.1), 0, 1536, 1792, None, None, 0, None), 1, b"max_displacement")
    for name in ("pdepth_flow_cost_volume_f32", "pdepth_flow_cost_volume_backward_f32", "pdepth_flow_cost_volume_backward_det_f32"):
        assert name in _native.EXPORTED_SYMBOLS and name in _native._ABSENT_FROM_EXPERIMENT_LIBS
    assert _native._SOURCE_OF_ENTRY["_flow_cost_volume_"] == "csrc/cost_volume.hip"
    assert _native._entry.__doc__ and next(src for part, src in _native._SOURCE_OF_ENTRY.items() if part in "pdepth_flow_cost_volume_f32") == "csrc/cost_volume.hip"
    assert lib.pdepth_abi_version() == 6
