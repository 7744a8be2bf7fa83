"""GPU suite: ops.flow_cost_volume (csrc/cost_volume.hip), forward and backward, against the float64 restatement of
tests/util_cost_volume.py; the tolerance of every comparison is util_flow.tol: twice the fp32 CPU composition's own error against
float64, with a floor of 8 eps32 times the largest value in play.

  forward     every case (util_cost_volume.CASES) and padding; the same bits from call to call
  gradients   grad_x1; grad_x2 by float atomics and by the integer sum; grad_flow on the kept pixels (util_flow.near_jump)
  bits        the deterministic backward twice; torch.use_deterministic_algorithms(True) selects it without the keyword
  non-finite  a NaN in x2 and an inf in x1 next to the border reach the outputs the composition of the existing device ops
              (flow_warp, correlation, leaky_relu) makes non-finite, and only those
  refusals    md = 5, H = 1 with a flow, a NaN slope
Every test prints the figures it asserts on.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdepth_amd import _native, ops
import util_cost_volume as U

pytestmark = pytest.mark.gpu

RUNS = [(c, p) for c in U.CASES for p in (U.PADS if c[2] else U.PADS[:1])]
_ids = lambda r: U.case_id(r[0]) + "-" + r[1]   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _device(case, dev, grad=False):
    x1, x2, flow, go, _ = U.inputs(case)
    t = [torch.from_numpy(v).to(dev).requires_grad_(grad) for v in (x1, x2)]
    f = torch.from_numpy(flow).to(dev).requires_grad_(grad) if flow is not None else None
    return t[0], t[1], f, torch.from_numpy(go).to(dev)


def _grads(case, pad, dev, det=None):
    x1, x2, flow, go = _device(case, dev, grad=True)
    out = ops.flow_cost_volume(x1, x2, flow, max_displacement=case[1], negative_slope=U.SLOPE, pad=pad, deterministic=det)
    wrt = (x1, x2) if flow is None else (x1, x2, flow)
    return torch.autograd.grad(out, wrt, go)


def _err(got, ref, keep=None):
    d = (got.double().cpu() - ref).abs()
    return float(d[keep].max() if keep is not None else d.max())


@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_forward(run, dev):
    case, pad = run
    ref = U.reference(case, pad)
    x1, x2, flow, _ = _device(case, dev)
    out = ops.flow_cost_volume(x1, x2, flow, max_displacement=case[1], negative_slope=U.SLOPE, pad=pad)
    got = _err(out, ref.out)
    print(f"forward {U.case_id(case)} {pad}: error {got:.2e}, fp32 composition {ref.err_out:.2e}, tolerance {ref.tol_out:.2e}")
    B, _, H, W = case[0]
    assert tuple(out.shape) == (B, (2 * case[1] + 1) ** 2, H, W) and out.dtype == torch.float32
    assert got <= ref.tol_out
    assert torch.equal(out, ops.flow_cost_volume(x1, x2, flow, max_displacement=case[1], negative_slope=U.SLOPE, pad=pad))


@pytest.mark.parametrize("det", (False, True), ids=("atomic", "det"))
@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_grad_x1_x2(run, det, dev):
    case, pad = run
    ref = U.reference(case, pad)
    g = _grads(case, pad, dev, det=det)
    e1, e2 = _err(g[0], ref.g_x1), _err(g[1], ref.g_x2)
    print(f"grads {U.case_id(case)} {pad} det={det}: grad_x1 error {e1:.2e} (fp32 autograd {ref.err_g_x1:.2e}, tolerance {ref.tol_g_x1:.2e}), "
          f"grad_x2 error {e2:.2e} (fp32 autograd {ref.err_g_x2:.2e}, tolerance {ref.tol_g_x2:.2e})")
    assert tuple(g[0].shape) == tuple(g[1].shape) == tuple(case[0])
    assert e1 <= ref.tol_g_x1 and e2 <= ref.tol_g_x2


@pytest.mark.parametrize("run", [r for r in RUNS if r[0][2]], ids=_ids)
def test_grad_flow(run, dev):
    case, pad = run
    ref = U.reference(case, pad)
    gf = _grads(case, pad, dev)[2]
    assert bool(ref.keep.any())
    got = _err(gf, ref.g_flow, ref.keep)
    print(f"grad_flow {U.case_id(case)} {pad}: error {got:.2e}, fp32 autograd {ref.err_g_flow:.2e}, tolerance {ref.tol_g_flow:.2e}; "
          f"kept {int(ref.keep.sum())} of {ref.keep.numel()}")
    assert bool(torch.isfinite(gf).all()) and got <= ref.tol_g_flow
    assert torch.equal(gf, _grads(case, pad, dev, det=True)[2])   # a per-owner sum: the same bits from either entry


@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_backward_bits(run, dev, monkeypatch):
    case, pad = run
    ref = U.reference(case, pad)
    a, b = _grads(case, pad, dev, det=True), _grads(case, pad, dev, det=True)
    atomic = _grads(case, pad, dev, det=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(a[0], atomic[0])   # grad_x1 is gathered: the same bits either way
    apart = float((a[1] - atomic[1]).abs().max())
    print(f"bits {U.case_id(case)} {pad}: integer sum twice equal; |integer sum - atomics| of grad_x2 {apart:.2e}, tolerance {ref.tol_g_x2:.2e}")
    assert apart <= ref.tol_g_x2
    # without the keyword the global switch decides, at the call
    seen = []
    real = _native.flow_cost_volume_backward
    monkeypatch.setattr(_native, "flow_cost_volume_backward", lambda *p, **k: (seen.append(k["deterministic"]), real(*p, **k))[1])
    torch.use_deterministic_algorithms(True)
    try:
        c = _grads(case, pad, dev)
    finally:
        torch.use_deterministic_algorithms(False)
    d = _grads(case, pad, dev)
    assert seen == [True, False] and all(torch.equal(p, q) for p, q in zip(a, c)) and float((d[1] - a[1]).abs().max()) <= ref.tol_g_x2


# the no-flow cases, and one at md = 1: two tile rows and three tile columns, ragged both ways; the second channel chunk holds one
# channel; the tile (18 x 18) is narrower than the kernel's static allocation (24 x 24)
GATHER_CASES = [c for c in U.CASES if not c[2]] + [((1, 9, 17, 35), 1, False)]


@pytest.mark.parametrize("case", GATHER_CASES, ids=U.case_id)
def test_gather_has_the_bits_of_the_correlation_backward(case, dev):
    """Without a flow, launch 1 of the backward IS the correlation's backward on grad_out (out > 0 ? 1 : slope): flow_cost_volume_bwd_kernel
    (csrc/cost_volume.hip) restates the displacement loop and the store of correlation_bwd_kernel (csrc/correlation.hip), in the same
    order, so both gradients agree bit for bit, and each gradient alone has the bits of its twin from the both-gradients call, on
    either entry."""
    shape, md, _ = case
    if case in U.CASES:
        x1, x2, _, go = _device(case, dev)
    else:
        g = torch.Generator().manual_seed(2990)
        x1, x2 = (torch.randn(*shape, generator=g).to(dev) for _ in range(2))
        go = torch.randn(shape[0], (2 * md + 1) ** 2, *shape[2:], generator=g).to(dev)
    out = ops.flow_cost_volume(x1, x2, None, max_displacement=md, negative_slope=U.SLOPE)

    def fused(**want):
        return _native.flow_cost_volume_backward(x1, x2, None, out, go, max_displacement=md, negative_slope=U.SLOPE, **want)[:2]

    def composed(**want):
        return _native.correlation_backward(x1, x2, torch.where(out > 0, go, go * U.SLOPE), md, 1, md, 1, 1, 1, **want)
    f, c = fused(), composed()
    alone = ((fused(want_x2=False)[0], f[0]), (fused(want_x1=False)[1], f[1]),
             (composed(want2=False)[0], c[0]), (composed(want1=False)[1], c[1]))
    apart = [int((p.view(torch.int32) != q.view(torch.int32)).sum()) for p, q in tuple(zip(f, c)) + alone]
    print(f"gather {U.case_id(case)}: elements with other bits, fused against correlation (grad_x1, grad_x2) {apart[:2]}, "
          f"each gradient alone against its twin (fused x1, x2; correlation x1, x2) {apart[2:]}")
    assert tuple(f[0].shape) == tuple(f[1].shape) == tuple(shape)
    assert all(torch.equal(p, q) for p, q in zip(f, c))
    assert all(torch.equal(p, q) for p, q in alone)


@pytest.mark.parametrize("pad", U.PADS)
def test_non_finite_reaches_what_the_composition_makes_non_finite(pad, dev):
    case = U.CASES[1]   # (2, 3, 19, 27), md = 4
    x1, x2, flow, _ = (None if v is None else v.clone() for v in _device(case, dev))
    x2[0, 1, 7, 11] = float("nan")
    x1[1, 2, 0, 25] = float("inf")    # next to the top and right borders: its displacements reach the zero padding
    x1[0, 0, 18, 1] = float("-inf")
    fused = ops.flow_cost_volume(x1, x2, flow, max_displacement=4, negative_slope=U.SLOPE, pad=pad)
    composed = F.leaky_relu(ops.correlation(x1, ops.flow_warp(x2, flow, pad=pad), 4, 1, 4, 1, 1, 1), U.SLOPE)
    bad_f, bad_c = ~torch.isfinite(fused), ~torch.isfinite(composed)
    worst = float((fused - composed)[~bad_c].abs().max())
    print(f"non-finite {pad}: {int(bad_f.sum())} fused, {int(bad_c.sum())} composed of {fused.numel()}; NaN {int(torch.isnan(fused).sum())} / "
          f"{int(torch.isnan(composed).sum())}; finite values apart by {worst:.2e}")
    assert torch.equal(bad_f, bad_c) and torch.equal(torch.isnan(fused), torch.isnan(composed))
    assert 2 * 81 <= int(bad_f.sum()) < fused.numel() // 4
    assert bool(bad_f[1, :, 0, 25].all()) and bool(bad_f[0, :, 18, 1].all()) and bool(torch.isnan(fused[1, 0, 0, 25]))
    assert worst <= 8 * U.EPS32 * float(x1[torch.isfinite(x1)].abs().max()) * float(x2[torch.isfinite(x2)].abs().max())


def test_refused_arguments(dev):
    x = torch.zeros(1, 2, 4, 6, device=dev)
    f = torch.zeros(1, 2, 4, 6, device=dev)
    with pytest.raises(RuntimeError, match="max_displacement must be 1..4"):
        ops.flow_cost_volume(x, x, f, max_displacement=5)
    with pytest.raises(RuntimeError, match="at least 2 with a flow"):
        ops.flow_cost_volume(x[:, :, :1], x[:, :, :1], f[:, :, :1])
    with pytest.raises(RuntimeError, match="negative_slope is NaN or negative"):
        ops.flow_cost_volume(x, x, f, negative_slope=float("nan"))
    with pytest.raises(RuntimeError, match="negative_slope is NaN or negative"):
        ops.flow_cost_volume(x, x, f, negative_slope=-0.1)
    with pytest.raises(RuntimeError, match="pad must be"):
        ops.flow_cost_volume(x, x, f, pad="reflect")
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.flow_cost_volume(x.double(), x.double(), f.double())
    # H = 1 without a flow is a shape like any other
    out = ops.flow_cost_volume(x[:, :, :1], x[:, :, :1])
    assert tuple(out.shape) == (1, 81, 1, 6) and float(out.abs().max()) == 0.0
    # the library itself refuses too, before any launch
    lib = _native.load()
    rc = lib.pdepth_flow_cost_volume_f32(x.data_ptr(), x.data_ptr(), f.data_ptr(), 1, 2, 4, 6, 5, 0.1, 0, x.data_ptr(), None)
    assert rc == 1 and b"max_displacement" in lib.pdepth_last_error()
    rc = lib.pdepth_flow_cost_volume_f32(x.data_ptr(), x.data_ptr(), f.data_ptr(), 1, 2, 1, 6, 4, 0.1, 0, x.data_ptr(), None)
    assert rc == 1 and b"at least 2 with a flow" in lib.pdepth_last_error()
    rc = lib.pdepth_flow_cost_volume_f32(x.data_ptr(), x.data_ptr(), f.data_ptr(), 1, 2, 4, 6, 4, float("nan"), 0, x.data_ptr(), None)
    assert rc == 1 and b"negative_slope" in lib.pdepth_last_error()
