"""CPU suite of flow_warp, the forward-backward check, the first-order smoothness and unFlowLoss: the float64 restatement the GPU
tests compare against (tests/util_flow.py) is checked against the reference's results (fixture g28_flow); then the interface, and
every refusal that is decided before a launch; last the register metadata of the new kernels."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import flow_loss as fl
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.utils import warp_utils as wu
import util_flow as U

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "probabilistic-depth_amd", "csrc")


def _close(mine, ref):
    """1e-9 of the largest value: the fixture keeps a float64 result as a float32 one plus a float32 difference."""
    return float((mine - ref).abs().max()) <= 1e-9 * max(1.0, float(ref.abs().max()))


def _sub(t):
    return torch.from_numpy(U.subset(t.detach().numpy()))


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.shape_key)
def test_warp_restatement_against_the_fixture(shape):
    c = U.cases()["warp_" + U.shape_key(shape)]
    x, flow, go, planted = U.warp_inputs(shape)
    assert np.array_equal(flow, c["flow"]) and np.array_equal(planted, c["planted"].astype(bool))   # the generator is the maker's
    B, C, H, W = shape
    ix, iy = U.positions(torch.from_numpy(flow).double())
    px, py = torch.from_numpy(U.chain(np.arange(W), flow[:, 0], W)), torch.from_numpy(U.chain(np.arange(H)[:, None], flow[:, 1], H))
    sel = torch.from_numpy(planted)
    if H * W >= 64:
        # what is planted is there, in the kernels' chain: integers, both boundaries with a neighbour on each side, all four exits.
        # The positions an fp32 flow can reach form a lattice of an ulp of the flow, on which 0, W - 1 or an integer need not lie:
        # "exactly" is the lattice point nearest to it, the neighbours are the next ones on either side.
        for p, size in ((px[sel], W), (py[sel], H)):
            step = 2 * size * U.EPS32
            assert bool((p.abs() <= step).any()) and bool(((p - (size - 1)).abs() <= step).any())
            assert bool(((p < 0) & (p > -1e-5)).any()) and bool(((p > 0) & (p < 1e-5)).any())
            assert bool(((p < size - 1) & (p > size - 1 - 1e-4)).any()) and bool(((p > size - 1) & (p < size - 1 + 1e-4)).any())
            assert bool((p < -1).any()) and bool((p > size).any()) and bool((p.abs() > 1e5).any())
            assert bool((((p - p.round()).abs() <= step) & (p > 0.5) & (p < size - 1.5)).any())
    assert float((px - ix).abs()[ix.abs() < 1e3].max()) < 1e-9   # (the restatement's float64 position is the chain's)
    for pad in U.PADS:
        tx, tf = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(flow).double().requires_grad_(True)
        out = U.flow_warp_ref(tx, tf, pad)
        gx, gf = torch.autograd.grad(out, (tx, tf), torch.from_numpy(go).double())
        assert _close(_sub(out), U.ref64(c, pad + ".out"))
        assert _close(_sub(gx), U.ref64(c, pad + ".grad_x"))
        keep = _sub((~U.near_jump(tf.detach(), pad)).unsqueeze(1).expand_as(gf).double()) > 0
        assert _close(_sub(gf)[keep], U.ref64(c, pad + ".grad_flow")[keep])
        # the share of samples the gradient's comparison leaves out, the planted ones aside
        free = ~sel
        assert float(U.near_jump(tf.detach(), pad)[free].double().mean()) <= 0.01


def test_non_finite_positions_have_no_tap():
    """The stated departure: value and both gradients are 0 where the position is NaN or infinite, in both paddings."""
    x = torch.randn(1, 2, 4, 5, dtype=torch.float64, requires_grad=True)
    flow = torch.zeros(1, 2, 4, 5, dtype=torch.float64)
    flow[0, 0, 1, 1], flow[0, 1, 2, 2], flow[0, 0, 3, 3] = float("nan"), float("inf"), float("-inf")
    flow.requires_grad_(True)
    for pad in U.PADS:
        out = U.flow_warp_ref(x, flow, pad)
        assert bool(torch.isfinite(out).all())
        for y, xx in ((1, 1), (2, 2), (3, 3)):
            assert float(out.detach()[0, :, y, xx].abs().max()) == 0.0
        gx, gf = torch.autograd.grad(out.sum(), (x, flow))
        assert bool(torch.isfinite(gx).all()) and float(gf[0, :, 1, 1].abs().max()) == 0.0


def test_smooth_restatement_against_the_fixture():
    c = U.cases()["smooth"]
    flo, image, alpha = U.smooth_inputs()
    assert np.array_equal(flo, c["flo"]) and np.array_equal(image, c["image"]) and alpha == float(c["alpha"])
    tf = torch.from_numpy(flo).double().requires_grad_(True)
    v = U.smooth_ref(tf, torch.from_numpy(image).double(), alpha)
    g = torch.autograd.grad(v, tf)[0]
    assert _close(v.detach().reshape(1), U.ref64(c, "value")) and _close(_sub(g), U.ref64(c, "grad"))
    assert float(flo[0, 0, 3, 5] - flo[0, 0, 3, 4]) == 0.0 and float(flo[1, 1, 6, 7] - flo[1, 1, 5, 7]) == 0.0   # sign(0) = 0 is exercised


@pytest.mark.parametrize("case", U.UNFLOW_CASES, ids=lambda c: U.unflow_name(*c))
def test_unflow_restatement_against_the_fixture(case):
    c, inp = U.cases()[U.unflow_name(*case)], U.cases()["unflow"]
    flows, target = U.unflow_inputs()
    assert np.array_equal(target, inp["target"]) and all(np.array_equal(f, inp[f"flow{i}"]) for i, f in enumerate(flows))
    assert [tuple(f.shape) for f in flows] == [(2, 4) + s for s in U.UNFLOW_SHAPES] and tuple(target.shape) == (2, 6, 24, 40)
    tfl = [torch.from_numpy(f).double().requires_grad_(True) for f in flows]
    vals, margin = U.unflow_ref(U.unflow_cfg(*case), tfl, torch.from_numpy(target).double())
    assert margin > 3e-4
    assert _close(torch.stack([v.detach() for v in vals]), U.ref64(c, "values"))
    for i, g in enumerate(torch.autograd.grad(vals[0], tfl)):
        assert float(g.abs().max()) > 0 and _close(_sub(g), U.ref64(c, f"grad{i}")), i


def test_fb_inputs_are_decisive():
    """The occluded share lies between 0.15 and 0.9 and at most 1 % of the pixels are within 1e-4 of the comparison."""
    for shape in U.FB_SHAPES:
        f12, f21 = (torch.from_numpy(v).double() for v in U.fb_inputs(shape))
        occ, m = U.fb_check_ref(f12, f21)
        assert 0.15 < float(occ.mean()) < 0.9 and float((m < 1e-4).double().mean()) <= 0.01
        assert torch.equal(occ, wu.get_occu_mask_bidirection(f12, f21))   # (the CPU composition, float64)


def test_reference_signatures():
    def names(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]
    E = inspect.Parameter.empty
    assert names(lb.gradient) == [("data", E)]
    assert names(lb.smooth_grad_1st) == [("flo", E), ("image", E), ("alpha", E)]
    assert names(fl.unFlowLoss.__init__) == [("self", E), ("cfg", E)]
    assert names(fl.unFlowLoss.forward) == [("self", E), ("output", E), ("target", E)]
    assert names(fl.unFlowLoss.loss_photomatric) == [("self", E), ("im1_scaled", E), ("im1_recons", E), ("occu_mask1", E)]
    assert names(fl.unFlowLoss.loss_smooth) == [("self", E), ("flow", E), ("im1_scaled", E)]
    assert names(wu.flow_warp) == [("x", E), ("flow12", E), ("pad", "border"), ("mode", "bilinear")]
    assert names(wu.get_occu_mask_bidirection) == [("flow12", E), ("flow21", E), ("scale", 0.01), ("bias", 0.5)]
    assert names(ops.flow_warp) == [("x", E), ("flow", E), ("pad", "border"), ("deterministic", None)]
    assert names(ops.flow_fb_check) == [("flow12", E), ("flow21", E), ("scale", 0.01), ("bias", 0.5)]
    assert names(ops.smooth_grad_1st) == [("flo", E), ("image", E), ("alpha", E)]
    d = torch.arange(24.0).view(1, 2, 3, 4) ** 2
    dx, dy = lb.gradient(d)
    assert tuple(dx.shape) == (1, 2, 3, 3) and tuple(dy.shape) == (1, 2, 2, 4)
    assert torch.equal(dx, d[..., 1:] - d[..., :-1]) and torch.equal(dy, d[:, :, 1:] - d[:, :, :-1])


def test_binding_refuses_before_any_launch():
    x, f = torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8)
    for call in (lambda: ops.flow_warp(x, f), lambda: ops.flow_warp(x, f, pad="zeros"),
                 lambda: ops.flow_warp(x, f.clone().requires_grad_(True)), lambda: ops.flow_fb_check(f, f),
                 lambda: ops.smooth_grad_1st(f, x, 10.0), lambda: ops.smooth_grad_1st(f.clone().requires_grad_(True), x, 10.0),
                 lambda: lb.smooth_grad_1st(f, x, 10.0),
                 lambda: fl.unFlowLoss(U.unflow_cfg(True, True, "border"))([torch.zeros(2, 4, 8, 8)], torch.zeros(2, 6, 8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match="pad must be 'border' or 'zeros'"):
        ops.flow_warp(x, f, pad="reflection")
    with pytest.raises(RuntimeError, match=r"flow must be \[2, 2, 8, 8\]"):
        ops.flow_warp(x, f[:, :1])
    with pytest.raises(RuntimeError, match="both must be at least 2"):
        ops.flow_warp(torch.zeros(1, 1, 1, 8), torch.zeros(1, 2, 1, 8))
    with pytest.raises(RuntimeError, match="x: expected float32, got torch.float64"):
        ops.flow_warp(x.double(), f)
    with pytest.raises(RuntimeError, match=r"flow12 must be \[B,2,H,W\]"):
        ops.flow_fb_check(x, x)
    with pytest.raises(RuntimeError, match="must share B, H and W"):
        ops.smooth_grad_1st(f, x[:, :, :7], 10.0)
    with pytest.raises(RuntimeError, match="image requires grad"):
        ops.smooth_grad_1st(f.clone().requires_grad_(True), x.clone().requires_grad_(True), 10.0)
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        ops.flow_warp(x.numpy(), f)
    # the CPU paths of warp_utils are the compositions they were
    assert tuple(wu.flow_warp(x, f).shape) == (2, 3, 8, 8) and tuple(wu.get_occu_mask_bidirection(f, f).shape) == (2, 1, 8, 8)


def test_entries_refuse_before_any_launch():
    """Every validation path of the new entries, with its code and message; no GPU is touched (the pointers are never read)."""
    lib = _native.load()
    fwd, bwd, det = lib.pdepth_flow_warp_f32, lib.pdepth_flow_warp_backward_f32, lib.pdepth_flow_warp_backward_det_f32
    fb, sm, smb = lib.pdepth_flow_fb_check_f32, lib.pdepth_loss_smooth1_f32, lib.pdepth_loss_smooth1_backward_f32
    q = lib.pdepth_flow_warp_backward_det_workspace_bytes

    def said(rc, code, words):
        return rc == code and words in lib.pdepth_last_error()

    for B, C, H, W in ((1, 1, 2, 2), (2, 3, 19, 27), (2, 192, 4, 8), (4, 3, 256, 832)):
        assert q(B, C, H, W) == (4 * B + 255) // 256 * 256 + (8 * B * C * H * W + 255) // 256 * 256
    for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 1, 4), (1, 1, 4, 1), (65536, 1, 4, 4), (1, 1, 1 << 16, 1 << 15)):
        assert q(*bad) == 0
    need = q(2, 3, 8, 8)
    assert need == 256 + 3072
    for args in ((None, 256, 512), (256, None, 512), (256, 512, None)):
        assert said(fwd(args[0], args[1], 2, 3, 8, 8, 0, args[2], None), 1, b"pdepth_flow_warp_f32: null pointer")
        assert said(bwd(*args, 2, 3, 8, 8, 0, 768, 1024, None), 1, b"pdepth_flow_warp_backward_f32: null pointer")
        assert said(det(*args, 2, 3, 8, 8, 0, 768, 1024, 4096, need, None), 1, b"pdepth_flow_warp_backward_det_f32: null pointer")
        assert said(fb(args[0], args[1], 2, 8, 8, 0.01, 0.5, args[2], None), 1, b"pdepth_flow_fb_check_f32: null pointer")
    assert said(bwd(256, 512, 768, 2, 3, 8, 8, 0, None, None, None), 1, b"no gradient requested")
    assert said(det(256, 512, 768, 2, 3, 8, 8, 0, None, None, 4096, need, None), 1, b"no gradient requested")
    for dims, words in (((0, 3, 8, 8), b"non-positive dimension"), ((2, 0, 8, 8), b"non-positive dimension"),
                        ((2, 3, 1, 8), b"H and W must be at least 2"), ((2, 3, 8, 1), b"H and W must be at least 2"),
                        ((65536, 3, 8, 8), b"B at most 65535"), ((1, 1, 1 << 16, 1 << 15), b"H*W must be at most 2^30")):
        assert said(fwd(256, 512, *dims, 0, 768, None), 1, words), dims
        assert said(bwd(256, 512, 768, *dims, 1, 1024, 1280, None), 1, words), dims
        assert said(det(256, 512, 768, *dims, 1, 1024, 1280, 4096, 1 << 40, None), 1, words), dims
    assert said(fb(256, 512, 2, 1, 8, 0.01, 0.5, 768, None), 1, b"H and W must be at least 2")
    assert said(fb(256, 512, 2, 8, 8, float("nan"), 0.5, 768, None), 1, b"scale or bias is NaN")
    for pad in (-1, 2, 7):
        assert said(fwd(256, 512, 2, 3, 8, 8, pad, 768, None), 1, b"unknown pad")
        assert said(bwd(256, 512, 768, 2, 3, 8, 8, pad, 1024, None, None), 1, b"unknown pad")
        assert said(det(256, 512, 768, 2, 3, 8, 8, pad, 1024, None, 4096, need, None), 1, b"unknown pad")
    # the workspace: missing, short, misaligned -- and not asked for when grad_x is not
    head = (256, 512, 768, 2, 3, 8, 8, 0, 1024, 1280)
    assert said(det(*head, None, 0, None), 3, b"needs 3328 bytes of workspace (got 0); query pdepth_flow_warp_backward_det_workspace_bytes()")
    assert said(det(*head, 4096, need - 1, None), 3, b"needs 3328 bytes of workspace (got 3327)")
    assert said(det(*head, 4096 + 64, need, None), 3, b"workspace must be 256-byte aligned")
    assert said(det(256, 512, 768, 2, 3, 8, 8, 2, 1024, 1280, None, 0, None), 1, b"unknown pad")   # arguments before the workspace
    # smooth1
    ws = lib.pdepth_loss_terms_workspace_bytes(2, 8, 8)
    assert said(sm(None, 256, 2, 2, 3, 8, 8, 10.0, 512, 4096, ws, None), 1, b"null pointer")
    assert said(sm(256, 512, 2, 2, 3, 8, 8, 10.0, None, 4096, ws, None), 1, b"null output pointer")
    assert said(sm(256, 512, 2, 0, 3, 8, 8, 10.0, 768, 4096, ws, None), 1, b"non-positive dimension")
    assert said(sm(256, 512, 2, 2, 3, 1, 8, 10.0, 768, 4096, ws, None), 1, b"H and W must be at least 2")
    assert said(sm(256, 512, 2, 2, 3, 8, 8, float("nan"), 768, 4096, ws, None), 1, b"alpha is NaN")
    assert said(sm(256, 512, 2, 2, 3, 8, 8, 10.0, 768, None, 0, None), 3, b"bytes of workspace")
    assert said(sm(256, 512, 2, 2, 3, 8, 8, 10.0, 768, 4096 + 32, ws, None), 3, b"256-byte aligned")
    assert said(smb(256, 512, None, 2, 2, 3, 8, 8, 10.0, 768, None), 1, b"null pointer")
    assert said(smb(256, 512, 768, 2, 2, 3, 8, 1, 10.0, 1024, None), 1, b"H and W must be at least 2")
    assert lib.pdepth_abi_version() == 6
    assert "csrc/flow_warp.hip" in _native._SOURCE_OF_ENTRY.values() and "csrc/loss_smooth1.hip" in _native._SOURCE_OF_ENTRY.values()
    for name in ("pdepth_flow_warp_f32", "pdepth_flow_warp_backward_f32", "pdepth_flow_warp_backward_det_workspace_bytes",
                 "pdepth_flow_warp_backward_det_f32", "pdepth_flow_fb_check_f32", "pdepth_loss_smooth1_f32",
                 "pdepth_loss_smooth1_backward_f32"):
        assert name in _native.EXPORTED_SYMBOLS and name in _native._ABSENT_FROM_EXPERIMENT_LIBS


def _metadata(name):
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc here")
    r = subprocess.run(["make", "-C", CSRC, name + ".s"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(CSRC, name + ".s")).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        block = m.group(0)
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_flow_kernels_no_spills_no_scratch():
    """Read from the code-object metadata of `make flow_warp.s` alone: the forward, the atomic scatter, the two passes of the
    integer scatter, the grad_flow gather, the check and the convert pass of the integer sum."""
    ks = _metadata("flow_warp")
    for part, n in (("flow_warp_kernel", 1), ("flow_warp_bwd_kernel", 1), ("flow_warp_bwd_det_kernel", 2), ("flow_warp_grad_flow_kernel", 1),
                    ("flow_fb_check_kernel", 1), ("det_convert_kernel", 1)):
        assert len([k for k in ks if part in k]) == n, (part, sorted(ks))
    assert len(ks) == 7
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256 and md["group_segment_fixed_size"] == 0, (name, md)
        assert md["vgpr_count"] <= 64, (name, md)   # eight waves per SIMD: the kernels hide gather latency by occupancy alone


def test_smooth1_kernels_no_spills_no_scratch():
    """`make loss_smooth1.s`: the forward, the backward and the fixed-order sum of the partial sums."""
    ks = _metadata("loss_smooth1")
    assert len([k for k in ks if "loss_smooth1_kernel" in k]) == 1 and len([k for k in ks if "loss_smooth1_bwd_kernel" in k]) == 1
    assert len([k for k in ks if "loss_terms_final_kernel" in k]) == 1 and len(ks) == 3, sorted(ks)
    for name, md in ks.items():
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (name, md)
