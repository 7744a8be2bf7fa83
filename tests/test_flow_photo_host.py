"""CPU suite of the fused photometric term of the flow loss (csrc/flow_photo.hip, ops.flow_photometric, unFlowLoss(cfg,
fused_photo=True)): the float64 restatement the GPU tests compare against (tests/util_flow_photo.py) is checked against the
reference's results (fixture g28_flow); then the input maker's cap, the interface, and the refusals that are decided before a
launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import flow_loss as fl
import util_flow as U
import util_flow_photo as P


@pytest.mark.parametrize("case", U.UNFLOW_CASES, ids=lambda c: U.unflow_name(*c))
def test_photo64_reproduces_the_fixture(case):
    """photo64, summed as unflow_ref sums it, against the reference's float64 run: 1e-9 of the largest value (the fixture keeps a
    float64 result as a float32 one plus a float32 difference)."""
    c = U.cases()[U.unflow_name(*case)]
    flows, target = U.unflow_inputs()
    tfl = [torch.from_numpy(f).double() for f in flows]
    vals = torch.stack(list(P.unflow_via_photo64(U.unflow_cfg(*case), tfl, torch.from_numpy(target).double())))
    ref = U.ref64(c, "values")
    err = float((vals - ref).abs().max())
    print(U.unflow_name(*case), "values", vals.tolist(), "fixture float64", ref.tolist(), "error %.2e" % err)
    assert err <= 1e-9 * max(1.0, float(ref.abs().max()))
    # and the nested function it was lifted from gives the same numbers
    own, _ = U.unflow_ref(U.unflow_cfg(*case), tfl, torch.from_numpy(target).double())
    assert float((vals - torch.stack(list(own))).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", P.SHAPES, ids=U.shape_key)
def test_maker_stays_within_the_cap(shape):
    t = P.make_inputs(shape)   # (asserts the cap itself)
    B, h, w = shape
    assert t["im"].shape == (B, 3, h, w) and t["other"].shape == (B, 3, h, w) and t["flow"].shape == (B, 2, h, w)
    assert t["mask"].shape == (B, 1, h, w) and set(np.unique(t["mask"])) <= {0.0, 1.0}
    zeros = float((t["mask"] == 0).mean())
    n_planted = int(t["planted"].sum())
    assert 0 < n_planted <= (B * h * w) // 2 and 0.05 <= zeros <= 0.35 and float(t["mask"].sum()) > 0
    for pad in P.PADS:
        share, keep = P.left_out(t, pad)
        jump = ~keep
        planted = torch.from_numpy(t["planted"])
        # the share is over the unplanted pixels alone: planted pixels that sit on a jump (they are aimed at one) do not count
        assert share == float(jump[~planted].double().mean())
        print(shape, pad, "zeros in the mask %.3f" % zeros, "planted", n_planted, "left out: unplanted share %.4f" % share,
              "planted pixels", int(jump[planted].sum()))
        assert share <= P.LEFT_OUT_CAP
    if B * h * w >= 64:   # what is planted is there: exits on every side, a huge flow, a pixel on a jump
        ix, iy = U.positions(torch.from_numpy(t["flow"]).double())
        sel = torch.from_numpy(t["planted"])
        for p, size in ((ix[sel], w), (iy[sel], h)):
            assert bool((p < -1).any()) and bool((p > size).any()) and bool((p.abs() > 1e5).any())
        assert int((~P.left_out(t, "border")[1])[sel].sum()) > 0


def test_interface():
    assert list(inspect.signature(fl.unFlowLoss.__init__).parameters) == ["self", "cfg"]   # the reference's, as it was
    assert list(inspect.signature(fl.unFlowLoss).parameters) == ["cfg", "fused_photo"]
    assert inspect.signature(fl.unFlowLoss).parameters["fused_photo"].default is False
    loss = fl.unFlowLoss(U.unflow_cfg(True, True, "border"))   # still takes one argument
    assert loss.fused_photo is False and fl.unFlowLoss(loss.cfg, fused_photo=True).fused_photo is True
    assert list(inspect.signature(ops.flow_photometric).parameters) == ["im", "other", "flow", "mask", "w_l1", "w_ssim", "w_ternary", "pad"]
    assert inspect.signature(ops.flow_photometric).parameters["pad"].default == "border"
    for name in ("pdepth_flow_photo_workspace_bytes", "pdepth_flow_photo_f32", "pdepth_flow_photo_backward_f32"):
        assert name in _native.EXPORTED_SYMBOLS


def test_refusals_before_a_launch():
    im, f, m = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8), torch.ones(1, 1, 8, 8)
    W3 = (0.15, 0.85, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_photometric(im, im, f, m, *W3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_photometric(im, im, f.clone().requires_grad_(True), m, *W3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fl.unFlowLoss(U.unflow_cfg(True, True, "border"), fused_photo=True)([torch.zeros(2, 4, 8, 8)], torch.zeros(2, 6, 8, 8))
    with pytest.raises(RuntimeError, match="pad must be 'border' or 'zeros'"):
        ops.flow_photometric(im, im, f, m, *W3, pad="reflection")
    with pytest.raises(RuntimeError, match=r"other must be \[1, 3, 8, 8\]"):
        ops.flow_photometric(im, torch.zeros(1, 3, 8, 9), f, m, *W3)
    with pytest.raises(RuntimeError, match=r"mask must be \[1, 1, 8, 8\]"):
        ops.flow_photometric(im, im, f, torch.ones(1, 8, 8), *W3)
    with pytest.raises(RuntimeError, match=r"flow must be \[1, 2, 8, 8\]"):
        ops.flow_photometric(im, im, torch.zeros(1, 4, 8, 8), m, *W3)
    with pytest.raises(RuntimeError, match=r"im must be \[B,3,H,W\]"):
        ops.flow_photometric(torch.zeros(1, 4, 8, 8), im, f, m, *W3)
    with pytest.raises(RuntimeError, match="H=2, W=9"):
        ops.flow_photometric(torch.zeros(1, 3, 2, 9), torch.zeros(1, 3, 2, 9), torch.zeros(1, 2, 2, 9), torch.ones(1, 1, 2, 9), *W3)
    for name in ("im", "other", "mask"):
        named = {"im": im, "other": im.clone(), "flow": f, "mask": m}
        named[name] = named[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=f"flow_photometric: {name} requires grad"):
            ops.flow_photometric(*named.values(), *W3)


def test_c_entries_validate_before_any_launch():
    """No GPU here: every call below must return its code from the argument checks (a launch would fail with code 2)."""
    lib = _native.load()
    buf = (ctypes.c_float * 4096)()
    aligned = (ctypes.addressof(buf) + 255) // 256 * 256   # a host address stands in: it is judged, never read
    p = ctypes.addressof(buf)
    err = lambda: lib.pdepth_last_error().decode()   # noqa: E731
    fwd, bwd = lib.pdepth_flow_photo_f32, lib.pdepth_flow_photo_backward_f32
    W3 = (0.15, 0.85, 0.5)
    need = lib.pdepth_flow_photo_workspace_bytes(1, 8, 8)
    assert need == 256 and lib.pdepth_flow_photo_workspace_bytes(2, 17, 130) == 512 and lib.pdepth_flow_photo_workspace_bytes(4, 256, 832) == 26624
    assert lib.pdepth_flow_photo_workspace_bytes(0, 8, 8) == 0 and lib.pdepth_flow_photo_workspace_bytes(1, 1, 8) == 0
    assert fwd(None, p, p, p, 1, 8, 8, 0, *W3, p, p, aligned, need, None) == 1 and "pdepth_flow_photo_f32: null pointer" in err()
    assert fwd(p, p, p, p, 1, 8, 8, 0, *W3, None, p, aligned, need, None) == 1 and "null output pointer" in err()
    assert fwd(p, p, p, p, 1, 8, 8, 2, *W3, p, p, aligned, need, None) == 1 and "unknown pad 2" in err()
    assert fwd(p, p, p, p, 1, 2, 9, 0, *W3, p, p, aligned, need, None) == 1 and "H=2, W=9" in err()
    assert fwd(p, p, p, p, 1, 2, 9, 0, 1.0, 0.0, 0.5, p, p, aligned, need, None) == 1 and "H=2, W=9" in err()
    assert fwd(p, p, p, p, 1, 1, 9, 0, 1.0, 0.0, 0.0, p, p, aligned, need, None) == 1 and "at least 2" in err()   # flow_warp's own
    assert fwd(p, p, p, p, 0, 8, 8, 0, *W3, p, p, aligned, need, None) == 1 and "non-positive dimension" in err()
    assert fwd(p, p, p, p, 5, 2048, 2048, 0, *W3, p, p, aligned, need, None) == 1 and "2^24" in err()
    assert fwd(p, p, p, p, 1, 8, 8, 0, *W3, p, p, aligned, need - 1, None) == 3 and "needs 256 bytes of workspace (got 255)" in err()
    assert fwd(p, p, p, p, 1, 8, 8, 0, *W3, p, p, None, need, None) == 3
    assert fwd(p, p, p, p, 1, 8, 8, 0, *W3, p, p, aligned + 4, need, None) == 3 and "256-byte aligned" in err()
    q = p + 64
    assert bwd(p, p, p, p, p, p, 1, 8, 8, 0, *W3, None, None) == 1 and "pdepth_flow_photo_backward_f32: null pointer" in err()
    assert bwd(p, p, p, p, None, p, 1, 8, 8, 0, *W3, q, None) == 1 and "null pointer" in err()
    assert bwd(p, p, p, p, p, p, 1, 8, 8, 7, *W3, q, None) == 1 and "unknown pad 7" in err()
    assert bwd(p, p, p, p, p, p, 1, 2, 9, 0, *W3, q, None) == 1 and "H=2, W=9" in err()
    assert bwd(p, p, p, p, p, p, 1, 8, 8, 0, *W3, p, None) == 1 and "may not alias" in err()
