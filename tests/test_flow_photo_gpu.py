"""GPU suite of the fused photometric term of the flow loss (csrc/flow_photo.hip; ops.flow_photometric; unFlowLoss(cfg,
fused_photo=True)).

Per shape of util_flow_photo.SHAPES, padding and weight set, with the incoming gradient 1.5: the mask count equals the mask's sum
exactly; value and gradient are measured against the float64 restatement util_flow_photo.photo64 next to the float32 composition's
own error against it (E_ref; the composition is today's unFlowLoss.loss_photomatric on ops.flow_warp, on the same device).  The
rule is the project's (tests/test_photo_gpu.py): the value may err by 2 E_ref + 4 ulp, a gradient element by 2 max E_ref + 1e-6 of
the largest gradient; gradient elements are compared everywhere but at the pixels whose own float64 sample position lies within
util_flow.NEAR of an integer or a clamp boundary (at most 1 % of the unplanted pixels: the maker asserts it).  Then: a weight that
is not > 0 removes its term, repeats, non-finite structure, views, unFlowLoss on every fixture case, 20 SGD steps, refusals.
Every test prints the figures it asserts on."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses.flow_loss import unFlowLoss
import util_flow as U
import util_flow_photo as P

pytestmark = pytest.mark.gpu

ALL = P.WEIGHTS[0]
G_OUT = 1.5
CASES = [(s, p, w) for s in P.SHAPES for p in P.PADS for w in P.WEIGHTS]
_ids = lambda c: "%s-%s-%s" % (U.shape_key(c[0]), c[1], "_".join(str(w) for w in c[2]))   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- the three sides: kernel, composition (float32, same device), restatement (float64, CPU) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape):
    cpu = P.make_inputs(shape)
    return cpu, {k: torch.from_numpy(v).cuda() for k, v in cpu.items() if k != "planted"}


def _kernel(t, flow, weights, pad):
    return ops.flow_photometric(t["im"], t["other"], flow, t["mask"], *weights, pad=pad)[0]


def _composition(t, flow, weights, pad):
    return unFlowLoss(P.cfg_of(weights, pad)).loss_photomatric(t["im"], ops.flow_warp(t["other"], flow, pad=pad), t["mask"])


def _run(fn, t, weights, pad, flow=None):
    """-> (value detached, gradient of the flow) of one float32 side."""
    x = (t["flow"] if flow is None else flow).clone().requires_grad_(True)
    value = fn(t, x, weights, pad)
    (value * G_OUT).backward()
    return value.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _reference(shape, pad, weights):
    """float64 value and gradient of the restatement, computed once on the CPU and left unchanged."""
    cpu, _ = _inputs(shape)
    im, other, mask = (torch.from_numpy(cpu[k]).double() for k in ("im", "other", "mask"))
    flow = torch.from_numpy(cpu["flow"]).double().requires_grad_(True)
    value = P.photo64(im, other, flow, mask, weights, pad)
    (g,) = torch.autograd.grad(value * G_OUT, flow)
    return value.detach(), g


# ---- 1: count ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", P.SHAPES, ids=U.shape_key)
def test_count_is_the_masks_sum(dev, shape):
    _, t = _inputs(shape)
    value, count = ops.flow_photometric(t["im"], t["other"], t["flow"], t["mask"], *ALL)
    print(shape, "count", float(count), "mask.sum()", float(t["mask"].sum()), "value", float(value))
    assert torch.equal(count, t["mask"].sum()) and count.dim() == 0 and not count.requires_grad
    assert value.dim() == 0 and value.dtype == torch.float32 and bool(torch.isfinite(value))


# ---- 2: value and gradient against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_against_float64(dev, case):
    shape, pad, weights = case
    cpu, t = _inputs(shape)
    v64, g64 = _reference(shape, pad, weights)
    (vk, gk), (vc, gc) = _run(_kernel, t, weights, pad), _run(_composition, t, weights, pad)
    assert bool(torch.isfinite(v64)) and bool(torch.isfinite(g64).all())
    err_k, e_ref = abs(float(vk) - float(v64)), abs(float(vc) - float(v64))
    ulp = float(np.spacing(np.float32(abs(float(v64)))))
    print(_ids(case), "value", float(vk), "float64", float(v64), "kernel error %.3e  E_ref %.3e  ulp %.3e" % (err_k, e_ref, ulp))
    share, keep = P.left_out(cpu, pad)
    keep = keep.unsqueeze(1).expand_as(g64)
    k, c = gk.double().cpu(), gc.double().cpu()
    assert k.shape == g64.shape and bool(torch.isfinite(k).all())
    ek, er, big = float((k - g64)[keep].abs().max()), float((c - g64)[keep].abs().max()), float(g64.abs().max())
    print(_ids(case), "gradient: kernel max error %.3e  E_ref max %.3e  largest gradient %.3e  left out %.4f" % (ek, er, big, share))
    assert share <= P.LEFT_OUT_CAP
    assert err_k <= 2 * e_ref + 4 * ulp, (case, err_k, e_ref, ulp)
    assert ek <= 2 * er + 1e-6 * big, (case, ek, er, big)


# ---- 3: a weight that is not > 0 removes its term --------------------------------------------------------------------------------------
def test_zero_weight_removes_its_term(dev):
    """Every term sees every pixel, so what is planted is a value only one chain turns into a NaN.  1e30 in `im` overflows the
    SSIM's second moments (inf - inf) and leaves |im - R| and the census chain (t / sqrt(0.81 + t^2) = 0 for t^2 = inf) finite;
    3e38 also overflows the gray value (inf / inf) and leaves the L1 term finite.  A NaN is seen by all three."""
    shape = (2, 19, 27)
    _, t = _inputs(shape)
    y, x = (t["mask"][0, 0, 2:-2, 2:-2] == 1).nonzero()[7].tolist()   # a seen pixel away from the border
    at = (0, 1, y + 2, x + 2)
    assert float(t["mask"][0, 0, y + 2, x + 2]) == 1.0

    def run(plant, weights):
        s = dict(t, im=t["im"].clone())
        s["im"][at] = plant
        value, g = _run(_kernel, s, weights, "border")
        want = _composition(s, s["flow"], weights, "border")
        print("plant", plant, "weights", weights, "value", float(value), "composition", float(want))
        assert bool(torch.isfinite(value)) == bool(torch.isfinite(want))
        return value, g

    for plant, off, on in ((1e30, (0.15, 0.0, 0.5), ALL), (1e30, (0.15, -1.0, 0.5), ALL), (3e38, (0.15, 0.0, 0.0), (0.15, 0.0, 0.5)),
                           (3e38, (0.15, float("nan"), -0.5), (0.15, 0.0, 0.5))):
        value, g = run(plant, off)
        assert bool(torch.isfinite(value)) and bool(torch.isfinite(g).all()), (plant, off)
        assert not bool(torch.isfinite(run(plant, on)[0])), (plant, on)   # the plant bites where the term is on
    # all three off: 0 / mean(m), whatever the images hold
    for weights in ((0.0, 0.0, 0.0), (-1.0, 0.0, float("nan"))):
        s = dict(t, im=t["im"].clone())
        s["im"][at] = float("nan")
        value, count = ops.flow_photometric(s["im"], s["other"], s["flow"], s["mask"], *weights)
        print("all off", weights, "value", float(value), "count", float(count))
        assert float(value) == 0.0 and torch.equal(count, t["mask"].sum())
        assert bool(torch.isnan(ops.flow_photometric(s["im"], s["other"], s["flow"], s["mask"], 1.0, 0.0, 0.0)[0]))


# ---- 4: the same bits twice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", P.PADS)
def test_repeats_carry_the_same_bits(dev, pad):
    _, t = _inputs((1, 17, 130))
    (v1, g1), (v2, g2) = _run(_kernel, t, ALL, pad), _run(_kernel, t, ALL, pad)
    torch.use_deterministic_algorithms(True)
    try:
        v3, g3 = _run(_kernel, t, ALL, pad)
    finally:
        torch.use_deterministic_algorithms(False)
    with torch.no_grad():
        v4 = _kernel(t, t["flow"], ALL, pad)
    assert torch.equal(v1, v2) and torch.equal(g1, g2) and torch.equal(v1, v3) and torch.equal(g1, g3) and torch.equal(v1, v4)


# ---- 5: masks and non-finite values ------------------------------------------------------------------------------------------------------
def test_nonfinite_structure(dev):
    shape = (2, 19, 27)
    _, t = _inputs(shape)
    for pad in P.PADS:
        flow = t["flow"].clone()
        flow[1, 0, 7, 11] = float("nan")   # no tap: R = 0 there, as ops.flow_warp
        (vk, gk), (vc, gc) = _run(_kernel, t, ALL, pad, flow=flow), _run(_composition, t, ALL, pad, flow=flow)
        print(pad, "NaN flow: value", float(vk), "composition", float(vc), "NaN gradients", int(torch.isnan(gk).sum()), int(torch.isnan(gc).sum()))
        assert bool(torch.isnan(vk)) == bool(torch.isnan(vc)) and torch.equal(torch.isnan(gk), torch.isnan(gc))
        assert abs(float(vk) - float(vc)) <= 1e-5 * abs(float(vc))
    # a NaN behind a zero mask: the products stay products
    deep = torch.nn.functional.max_pool2d(t["mask"], 5, 1, 2)[0, 0, 2:-2, 2:-2] == 0   # unseen, and so is everything within 2 pixels
    zero = deep.nonzero()[0] + 2
    other = t["other"].clone()
    other[0, 2, zero[0], zero[1]] = float("nan")
    flow0 = torch.zeros_like(t["flow"])   # (every pixel samples within a pixel of itself: only unseen pixels read the NaN)
    s = dict(t, other=other)
    vk, vc = _kernel(s, flow0, ALL, "border"), _composition(s, flow0, ALL, "border")
    print("NaN behind a zero mask: value", float(vk), "composition", float(vc))
    assert bool(torch.isnan(vk)) and bool(torch.isnan(vc))
    # an empty mask: 0 / 0
    value, count = ops.flow_photometric(t["im"], t["other"], t["flow"], torch.zeros_like(t["mask"]), *ALL)
    print("empty mask: value", float(value), "count", float(count))
    assert float(count) == 0.0 and bool(torch.isnan(value))


# ---- 6: a view of a wider tensor ---------------------------------------------------------------------------------------------------------
def test_view_gives_the_bits_of_its_copy(dev):
    shape = (2, 19, 27)
    _, t = _inputs(shape)
    v0, g0 = _run(_kernel, t, ALL, "border")
    wide = torch.zeros(2, 4, 19, 54, device=dev)
    wide[:, 1:3, :, ::2] = t["flow"]
    wide.requires_grad_(True)
    view = wide[:, 1:3, :, ::2]
    assert not view.is_contiguous()
    wide_im = torch.zeros(2, 3, 19, 54, device=dev)
    wide_im[..., 1::2] = t["im"]
    value = ops.flow_photometric(wide_im[..., 1::2], t["other"], view, t["mask"], *ALL)[0]
    (value * G_OUT).backward()
    assert torch.equal(value.detach(), v0) and torch.equal(wide.grad[:, 1:3, :, ::2], g0)
    assert not bool(wide.grad[:, 1:3, :, 1::2].any()) and not bool(wide.grad[:, 0].any()) and not bool(wide.grad[:, 3].any())


# ---- 7: unFlowLoss(cfg, fused_photo=True) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unflow_reference(case):
    flows, target = U.unflow_inputs()
    tfl = [torch.from_numpy(f).double().requires_grad_(True) for f in flows]
    vals, _ = U.unflow_ref(U.unflow_cfg(*case), tfl, torch.from_numpy(target).double())
    return torch.stack([v.detach() for v in vals]), torch.autograd.grad(vals[0], tfl)


def _unflow_run(dev, case, **switch):
    flows, target = U.unflow_inputs()
    tfl = [torch.from_numpy(f).to(dev).requires_grad_(True) for f in flows]
    vals = unFlowLoss(U.unflow_cfg(*case), **switch)(tfl, torch.from_numpy(target).to(dev))
    return vals, torch.autograd.grad(vals[0], tfl)


@pytest.mark.parametrize("case", U.UNFLOW_CASES, ids=lambda c: U.unflow_name(*c))
def test_unflow_loss_fused(case, dev, monkeypatch):
    c = U.cases()[U.unflow_name(*case)]
    v64, g64 = _unflow_reference(case)
    flows, _ = U.unflow_inputs()
    base_vals, base_grads = _unflow_run(dev, case)
    off_vals, off_grads = _unflow_run(dev, case, fused_photo=False)
    assert all(torch.equal(a, b) for a, b in zip(base_vals, off_vals)) and all(torch.equal(a, b) for a, b in zip(base_grads, off_grads))
    calls = []
    for name in ("flow_photo", "flow_photo_backward", "ssim", "ternary", "flow_warp"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    vals, grads = _unflow_run(dev, case, fused_photo=True)
    n = 3 * (2 if case[1] else 1)   # levels x directions
    print(U.unflow_name(*case), "native calls with the switch on:", {k: calls.count(k) for k in sorted(set(calls))})
    assert calls == ["flow_photo"] * n + ["flow_photo_backward"] * n, calls
    del calls[:]
    _unflow_run(dev, case)
    assert calls.count("flow_photo") == 0 and calls.count("flow_warp") == n and calls.count("ssim") == n and calls.count("ternary") == n
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


# ---- 8: twenty SGD steps -----------------------------------------------------------------------------------------------------------------
def _train(dev, steps=20, lr=20.0):
    target = torch.from_numpy(U.train_images()).to(dev)
    flows = [torch.zeros(2, 4, h, w, device=dev, requires_grad=True) for h, w in U.UNFLOW_SHAPES]
    opt = torch.optim.SGD(flows, lr=lr)
    loss = unFlowLoss(U.unflow_cfg(False, True, "border"), fused_photo=True)
    totals = []
    for _ in range(steps):
        opt.zero_grad()
        total = loss(flows, target)[0]
        total.backward()
        opt.step()
        totals.append(total.detach().clone())
    return torch.stack(totals)


def test_unflow_fused_trains_and_repeats(dev):
    a, b = _train(dev), _train(dev)
    print("unFlowLoss(fused_photo=True), 20 SGD steps:", [round(float(v), 5) for v in a])
    assert bool(torch.isfinite(a).all()) and float(a[-1]) < float(a[0])
    assert torch.equal(a, b)


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(dev):
    _, t = _inputs((2, 6, 10))
    args = (t["im"], t["other"], t["flow"], t["mask"])
    thin = [torch.rand(1, c, 2, 9, device=dev) for c in (3, 3, 2, 1)]
    with pytest.raises(RuntimeError, match="H=2, W=9"):
        ops.flow_photometric(*thin, *ALL)
    with pytest.raises(RuntimeError, match="H=2, W=9"):
        ops.flow_photometric(*thin, 1.0, 0.0, 0.5)
    value = ops.flow_photometric(*thin, 1.0, 0.0, 0.0)[0]   # the L1 term alone needs no window
    assert bool(torch.isfinite(value))
    with pytest.raises(RuntimeError, match="pad must be 'border' or 'zeros'"):
        ops.flow_photometric(*args, *ALL, pad="reflection")
    with pytest.raises(RuntimeError, match=r"other must be \[2, 3, 6, 10\]"):
        ops.flow_photometric(args[0], thin[1], *args[2:], *ALL)
    with pytest.raises(RuntimeError, match=r"flow must be \[2, 2, 6, 10\]"):
        ops.flow_photometric(*args[:2], t["flow"][:, :1], args[3], *ALL)
    with pytest.raises(RuntimeError, match=r"mask must be \[2, 1, 6, 10\]"):
        ops.flow_photometric(*args[:3], t["mask"][:, 0], *ALL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_photometric(args[0].cpu(), *args[1:], *ALL)
    for name in ("im", "other", "mask"):
        named = dict(zip(("im", "other", "flow", "mask"), args))
        named[name] = named[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=f"flow_photometric: {name} requires grad"):
            ops.flow_photometric(*named.values(), *ALL)
    x = t["flow"].clone().requires_grad_(True)   # once_differentiable: a second-order gradient raises, it is not a constant
    (g,) = torch.autograd.grad(ops.flow_photometric(args[0], args[1], x, args[3], *ALL)[0], x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # the C entries, past the binding's own checks
    lib = _native.load()
    out = torch.empty(2, device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    ptrs = [a.contiguous().data_ptr() for a in args]
    tail = (out[0:].data_ptr(), out[1:].data_ptr(), ws.data_ptr())
    err = lambda: lib.pdepth_last_error()   # noqa: E731
    assert lib.pdepth_flow_photo_workspace_bytes(2, 6, 10) == 256
    assert lib.pdepth_flow_photo_f32(*ptrs, 2, 6, 10, 0, *ALL, *tail, 255, None) == 3 and b"got 255" in err()
    assert lib.pdepth_flow_photo_f32(*ptrs, 2, 6, 10, 3, *ALL, *tail, 256, None) == 1 and b"unknown pad 3" in err()
    assert lib.pdepth_flow_photo_f32(*ptrs, 2, 2, 30, 0, *ALL, *tail, 256, None) == 1 and b"H=2, W=30" in err()
    assert lib.pdepth_flow_photo_f32(*ptrs, 2, 1, 60, 0, 1.0, 0.0, 0.0, *tail, 256, None) == 1 and b"at least 2" in err()
    assert lib.pdepth_flow_photo_f32(ptrs[0], None, *ptrs[2:], 2, 6, 10, 0, *ALL, *tail, 256, None) == 1 and b"null pointer" in err()
    g = torch.empty(2, 2, 6, 10, device=dev)
    back = (out[1:].data_ptr(), out[0:].data_ptr(), 2, 6, 10)
    assert lib.pdepth_flow_photo_backward_f32(*ptrs, *back, 5, *ALL, g.data_ptr(), None) == 1 and b"unknown pad 5" in err()
    assert lib.pdepth_flow_photo_backward_f32(*ptrs, *back, 0, *ALL, None, None) == 1 and b"null pointer" in err()
    assert lib.pdepth_flow_photo_f32(*ptrs, 2, 6, 10, 0, *ALL, *tail, 256, None) == 0   # and the call these were variations of runs
    assert lib.pdepth_flow_photo_backward_f32(*ptrs, *back, 0, *ALL, g.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], ops.flow_photometric(*args, *ALL)[0])
