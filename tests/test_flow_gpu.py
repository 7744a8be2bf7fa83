"""GPU suite of flow_warp, the forward-backward check, the first-order smoothness (csrc/flow_warp.hip, csrc/loss_smooth1.hip) and
unFlowLoss against the float64 restatement of tests/util_flow.py and the fixture g28_flow.

The contract (include/pdepth.h).  A tolerance is twice the error of the reference's own fp32 arithmetic against the
same float64 values -- the factor 2 for an equally valid fp32 order, fused or not -- and at least 8 eps32 times the largest value
in play (util_flow.tol):
  forward     both paddings; the fp32 reference is the torch composition of utils/warp_utils.flow_warp, run on the CPU here;
  grad_x      float atomics and the integer sum alike; the fp32 reference is torch's CPU autograd of that composition;
  grad_flow   the same, without the samples whose float64 position lies within util_flow.NEAR of an integer or a clamp boundary,
              where the derivative jumps; at most 1 % of the samples that are not planted may be left out;
  bits        the integer sum twice; torch.use_deterministic_algorithms(True) selects it without the keyword;
  check       the float64 mask at every pixel whose float64 margin |lhs - rhs| is at least 1e-4; at most 1 % are not;
  smooth      value and gradient, floor 16 eps32 relative; the same bits twice;
  unFlowLoss  every fixture case, four values and every level's gradient, the fp32 reference being the fixture's own fp32 run;
              20 SGD steps from a zero pyramid lower the total, bit for bit alike in two deterministic runs.
Every test prints the figures it asserts on."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.flow_loss import unFlowLoss
from pdepth_amd.utils import warp_utils as wu
import util_flow as U

pytestmark = pytest.mark.gpu

WARP_CASES = [(s, p) for s in U.SHAPES for p in U.PADS]
_ids = lambda c: U.shape_key(c[0]) + "-" + c[1]   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- references, computed once on the CPU and left unchanged ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warp_reference(shape, pad):
    """float64 out / grad_x / grad_flow of the restatement, the errors of the fp32 CPU composition against them, the samples the
    grad_flow comparison keeps [B,H,W], the share of unplanted samples it leaves out."""
    x, flow, go, planted = U.warp_inputs(shape)
    tx, tf = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(flow).double().requires_grad_(True)
    out = U.flow_warp_ref(tx, tf, pad)
    gx, gf = torch.autograd.grad(out, (tx, tf), torch.from_numpy(go).double())
    sx, sf = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(flow).requires_grad_(True)
    o32 = wu.flow_warp(sx, sf, pad=pad)   # (CPU tensors: the torch composition)
    gx32, gf32 = torch.autograd.grad(o32, (sx, sf), torch.from_numpy(go))
    jump = U.near_jump(tf.detach(), pad)
    keep = ~jump
    free = ~torch.from_numpy(planted)
    err = {"out": float((o32.detach().double() - out.detach()).abs().max()), "grad_x": float((gx32.double() - gx).abs().max()),
           "grad_flow": float((gf32.double() - gf)[keep.unsqueeze(1).expand_as(gf)].abs().max())}
    return {"out": out.detach(), "grad_x": gx, "grad_flow": gf, "err": err, "keep": keep,
            "left_out": float(jump[free].double().mean()), "planted_left_out": int(jump[~free].sum())}


def _warp_device(shape, dev, grad=False):
    x, flow, go, _ = U.warp_inputs(shape)
    x, flow, go = (torch.from_numpy(v).to(dev) for v in (x, flow, go))
    return (x.requires_grad_(grad), flow.requires_grad_(grad), go)


@pytest.mark.parametrize("case", WARP_CASES, ids=_ids)
def test_forward(case, dev):
    shape, pad = case
    ref = _warp_reference(shape, pad)
    x, flow, _ = _warp_device(shape, dev)
    out = ops.flow_warp(x, flow, pad=pad)
    tol = U.tol(ref["err"]["out"], x.abs().max())
    got = float((out.double().cpu() - ref["out"]).abs().max())
    print(f"forward {shape} {pad}: error {got:.2e}, fp32 composition {ref['err']['out']:.2e}, tolerance {tol:.2e}")
    assert tuple(out.shape) == tuple(shape) and out.dtype == torch.float32 and got <= tol
    assert torch.equal(out, ops.flow_warp(x, flow, pad=pad))


@pytest.mark.parametrize("det", (False, True), ids=("atomic", "det"))
@pytest.mark.parametrize("case", WARP_CASES, ids=_ids)
def test_grad_x(case, det, dev):
    shape, pad = case
    ref = _warp_reference(shape, pad)
    x, flow, go = _warp_device(shape, dev, grad=True)
    (gx,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad, deterministic=det), x, go)
    tol = U.tol(ref["err"]["grad_x"], go.abs().max())
    got = float((gx.double().cpu() - ref["grad_x"]).abs().max())
    print(f"grad_x {shape} {pad} det={det}: error {got:.2e}, fp32 autograd {ref['err']['grad_x']:.2e}, tolerance {tol:.2e}")
    assert tuple(gx.shape) == tuple(shape) and got <= tol


@pytest.mark.parametrize("case", WARP_CASES, ids=_ids)
def test_grad_flow(case, dev):
    shape, pad = case
    ref = _warp_reference(shape, pad)
    x, flow, go = _warp_device(shape, dev, grad=True)
    (gf,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad), flow, go)
    keep = ref["keep"].unsqueeze(1).expand_as(ref["grad_flow"])
    tol = U.tol(ref["err"]["grad_flow"], ref["grad_flow"][keep].abs().max())
    got = float((gf.double().cpu() - ref["grad_flow"])[keep].abs().max())
    print(f"grad_flow {shape} {pad}: error {got:.2e}, fp32 autograd {ref['err']['grad_flow']:.2e}, tolerance {tol:.2e}; left out "
          f"{100 * ref['left_out']:.2f} % of the unplanted samples and {ref['planted_left_out']} planted ones")
    assert ref["left_out"] <= 0.01 and bool(keep.any())
    assert bool(torch.isfinite(gf).all()) and got <= tol
    # the same bits from call to call (a per-owner sum), and from the deterministic entry
    x2, flow2, _ = _warp_device(shape, dev, grad=True)
    (again,) = torch.autograd.grad(ops.flow_warp(x2, flow2, pad=pad, deterministic=True), flow2, go)
    assert torch.equal(gf, again)


@pytest.mark.parametrize("case", WARP_CASES, ids=_ids)
def test_scatter_determinism(case, dev, monkeypatch):
    shape, pad = case
    ref = _warp_reference(shape, pad)
    x, flow, go = _warp_device(shape, dev, grad=True)
    (a,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad, deterministic=True), x, go)
    (b,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad, deterministic=True), x, go)
    (atomic,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad, deterministic=False), x, go)
    assert torch.equal(a, b)
    tol = U.tol(ref["err"]["grad_x"], go.abs().max())
    assert float((a - atomic).abs().max()) <= tol
    # without the keyword the global switch decides, at the call
    seen = []
    real = _native.flow_warp_backward
    monkeypatch.setattr(_native, "flow_warp_backward", lambda *p, **k: (seen.append(k["deterministic"]), real(*p, **k))[1])
    torch.use_deterministic_algorithms(True)
    try:
        out = ops.flow_warp(x, flow, pad=pad)
    finally:
        torch.use_deterministic_algorithms(False)
    (c,) = torch.autograd.grad(out, x, go)
    (d,) = torch.autograd.grad(ops.flow_warp(x, flow, pad=pad), x, go)
    assert seen == [True, False] and torch.equal(c, a) and float((d - a).abs().max()) <= tol


def test_item_independence_and_non_finite(dev):
    """An item's deterministic grad_x does not depend on its neighbours in the batch; a non-finite flow gives 0 (value, gradients) at
    its own pixel and nothing else changes."""
    shape = U.SHAPES[1]
    x, flow, go = _warp_device(shape, dev)
    for pad in U.PADS:
        gx, gf = _native.flow_warp_backward(x, flow, go, pad, deterministic=True)
        g1, f1 = _native.flow_warp_backward(x[1:], flow[1:], go[1:], pad, deterministic=True)
        assert torch.equal(gx[1:], g1) and torch.equal(gf[1:], f1)
        bad = flow.clone()
        bad[0, 0, 5, 6], bad[0, 1, 7, 8], bad[1, 0, 9, 10] = float("nan"), float("inf"), float("-inf")
        out, base = ops.flow_warp(x, bad, pad=pad), ops.flow_warp(x, flow, pad=pad)
        hit = torch.zeros(shape[0], 1, shape[2], shape[3], dtype=torch.bool, device=dev)
        hit[0, 0, 5, 6] = hit[0, 0, 7, 8] = hit[1, 0, 9, 10] = True
        assert torch.equal(out, torch.where(hit, torch.zeros_like(base), base))
        gxb, gfb = _native.flow_warp_backward(x, bad, go, pad, deterministic=True)
        gz = go * (~hit)   # what the samples without a tap would have scattered is missing, nothing else
        gxz, _ = _native.flow_warp_backward(x, flow, gz, pad, deterministic=True)
        assert torch.equal(gxb, gxz) and bool(torch.isfinite(gfb).all()) and float(gfb[hit.expand_as(gfb)].abs().max()) == 0.0


@pytest.mark.parametrize("shape", U.FB_SHAPES, ids=U.shape_key)
def test_fb_check(shape, dev):
    f12, f21 = (torch.from_numpy(v) for v in U.fb_inputs(shape))
    occ64, margin = U.fb_check_ref(f12.double(), f21.double())
    occ = ops.flow_fb_check(f12.to(dev), f21.to(dev))
    decided = margin >= 1e-4
    share, excepted = float(occ64.mean()), float((~decided).double().mean())
    wrong = int((occ.cpu() != occ64)[decided].sum())
    print(f"fb_check {shape}: occluded {share:.2f}, within the margin {100 * excepted:.2f} %, wrong {wrong}")
    assert tuple(occ.shape) == (shape[0], 1) + tuple(shape[1:]) and occ.dtype == torch.float32 and not occ.requires_grad
    assert excepted <= 0.01 and 0.15 < share < 0.9 and wrong == 0
    assert bool(((occ == 0) | (occ == 1)).all())
    # flows that require grad: the mask is a constant
    assert not ops.flow_fb_check(f12.to(dev).requires_grad_(True), f21.to(dev).requires_grad_(True)).requires_grad


def test_smooth_grad_1st(dev):
    flo, image, alpha = U.smooth_inputs()
    t64 = torch.from_numpy(flo).double().requires_grad_(True)
    v64 = U.smooth_ref(t64, torch.from_numpy(image).double(), alpha)
    (g64,) = torch.autograd.grad(v64, t64)
    t32 = torch.from_numpy(flo).requires_grad_(True)
    v32 = U.smooth_ref(t32, torch.from_numpy(image), alpha)   # (the fp32 torch composition, on the CPU)
    (g32,) = torch.autograd.grad(v32, t32)
    td, im = torch.from_numpy(flo).to(dev).requires_grad_(True), torch.from_numpy(image).to(dev)
    v = ops.smooth_grad_1st(td, im, alpha)
    (g,) = torch.autograd.grad(v, td)
    v64, v32 = v64.detach(), v32.detach()
    tol_v = U.tol(abs(float(v32) - float(v64)), abs(float(v64)), floor_eps=16)
    tol_g = U.tol(float((g32.double() - g64).abs().max()), float(g64.abs().max()), floor_eps=16)
    ev, eg = abs(float(v.detach()) - float(v64)), float((g.double().cpu() - g64).abs().max())
    print(f"smooth_grad_1st: value error {ev:.2e} (tolerance {tol_v:.2e}), gradient error {eg:.2e} (tolerance {tol_g:.2e})")
    assert v.dim() == 0 and v.dtype == torch.float32 and tuple(g.shape) == U.SMOOTH_SHAPE
    assert ev <= tol_v and eg <= tol_g
    v2 = lb.smooth_grad_1st(td, im, alpha)
    (g2,) = torch.autograd.grad(v2, td)
    assert torch.equal(v, v2) and torch.equal(g, g2) and torch.equal(v.detach(), ops.smooth_grad_1st(td.detach(), im, alpha))
    with pytest.raises(RuntimeError, match="image requires grad"):
        ops.smooth_grad_1st(td, im.clone().requires_grad_(True), alpha)


@functools.lru_cache(maxsize=None)
def _unflow_reference(case):
    flows, target = U.unflow_inputs()
    tfl = [torch.from_numpy(f).double().requires_grad_(True) for f in flows]
    vals, _ = U.unflow_ref(U.unflow_cfg(*case), tfl, torch.from_numpy(target).double())
    return torch.stack([v.detach() for v in vals]), torch.autograd.grad(vals[0], tfl)


@pytest.mark.parametrize("case", U.UNFLOW_CASES, ids=lambda c: U.unflow_name(*c))
def test_unflow_loss(case, dev):
    c = U.cases()[U.unflow_name(*case)]
    v64, g64 = _unflow_reference(case)
    flows, target = U.unflow_inputs()
    tfl = [torch.from_numpy(f).to(dev).requires_grad_(True) for f in flows]
    vals = unFlowLoss(U.unflow_cfg(*case))(tfl, torch.from_numpy(target).to(dev))
    grads = torch.autograd.grad(vals[0], tfl)
    assert len(vals) == 4 and all(v.dim() == 0 for v in vals)
    ok = True
    for i, (v, name) in enumerate(zip(vals, ("total", "warp", "smooth", "mean |flow|"))):
        ref_err = abs(float(c["values32"][i]) - float(v64[i]))
        tol, got = U.tol(ref_err, abs(float(v64[i]))), abs(float(v.detach()) - float(v64[i]))
        print(f"{U.unflow_name(*case)} {name}: error {got:.2e}, fixture fp32 {ref_err:.2e}, tolerance {tol:.2e}")
        ok = ok and got <= tol
    for i, g in enumerate(grads):
        ref_err = float((torch.from_numpy(c[f"grad{i}32"]).double() - g64[i]).abs().max())   # (kept whole: every element)
        tol, got = U.tol(ref_err, float(g64[i].abs().max())), float((g.double().cpu() - g64[i]).abs().max())
        print(f"{U.unflow_name(*case)} grad level {i}: error {got:.2e}, fixture fp32 {ref_err:.2e}, tolerance {tol:.2e}")
        ok = ok and tuple(g.shape) == tuple(flows[i].shape) and got <= tol
    assert ok


def _train(dev, steps=20, lr=20.0):
    """SGD on a raw three-level pyramid from zero; the totals, as the tensors the loss returned."""
    target = torch.from_numpy(U.train_images()).to(dev)
    flows = [torch.zeros(2, 4, h, w, device=dev, requires_grad=True) for h, w in U.UNFLOW_SHAPES]
    opt = torch.optim.SGD(flows, lr=lr)
    loss = unFlowLoss(U.unflow_cfg(False, True, "border"))
    totals = []
    for _ in range(steps):
        opt.zero_grad()
        total = loss(flows, target)[0]
        total.backward()
        opt.step()
        totals.append(total.detach().clone())
    return torch.stack(totals)


def test_unflow_trains_and_repeats(dev):
    torch.use_deterministic_algorithms(True)
    try:
        a, b = _train(dev), _train(dev)
    finally:
        torch.use_deterministic_algorithms(False)
    print("unFlowLoss, 20 SGD steps:", [round(float(v), 5) for v in a])
    assert bool(torch.isfinite(a).all()) and float(a[-1]) < float(a[0])
    assert torch.equal(a, b)


def test_warp_utils_dispatch(dev):
    shape = U.SHAPES[1]
    x, flow, _ = _warp_device(shape, dev)
    for pad in U.PADS:
        assert torch.equal(wu.flow_warp(x, flow, pad=pad), ops.flow_warp(x, flow, pad=pad))
    assert torch.equal(wu.flow_warp(x, flow), ops.flow_warp(x, flow, pad="border"))
    f12, f21 = (torch.from_numpy(v).to(dev) for v in U.fb_inputs(U.FB_SHAPES[0]))
    assert torch.equal(wu.get_occu_mask_bidirection(f12, f21), ops.flow_fb_check(f12, f21))
    assert torch.equal(wu.get_occu_mask_bidirection(f12, f21, 0.05, 1.0), ops.flow_fb_check(f12, f21, scale=0.05, bias=1.0))
    # what stays the torch composition: nearest, other dtypes
    near = wu.flow_warp(x, flow, pad="zeros", mode="nearest")
    assert tuple(near.shape) == tuple(shape) and bool(torch.isin(near[near != 0], x).all())   # (values of x, not blends)
    assert wu.flow_warp(x.double(), flow.double()).dtype == torch.float64
    # differentiable through the dispatch
    fl = flow.clone().requires_grad_(True)
    wu.flow_warp(x, fl).sum().backward()
    assert fl.grad is not None and bool(torch.isfinite(fl.grad).all())
