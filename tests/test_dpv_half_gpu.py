"""GPU suite: the DPV reductions on fp16 / bf16 logits (csrc/dpv_half.hip, pdepth_dpv_reduce_ex_lp / _backward_lp).

The yardstick is the fp32 path on the widened input, which other tests hold to the float64 oracle: the forward must give its
bits (the cast is the kernel's load, which is exact), prob in the half type and the backward's g_logits its values rounded
once.  One independent check against float64 on finite inputs, with the tolerances of
tests/test_hip_parity.py::test_dpv_reduce_shapes_and_properties."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from util import DEPTH_ATOL

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (B, D, H, W), the view starts one element into its storage
SHAPES = [
    ((2, 64, 8, 36), False),    # two workgroups, the second partial; the second item's offsets; quarter at 2 x 9
    ((1, 7, 4, 8), False),      # planes past D in an 8-plane lane
    ((1, 33, 4, 64), False),    # 16 planes per lane, with fill
    ((1, 128, 4, 64), False),   # 32 planes per lane
    ((1, 130, 4, 16), False),   # D > 128: the any-shape kernel
    ((1, 16, 5, 7), False),     # H W % 4 != 0: the any-shape kernel
    ((1, 16, 4, 16), True),     # 2-byte misalignment: the any-shape kernel in the wave layout's order
]
IDS = ["%dx%dx%dx%d%s" % (s + ("-odd" if o else "",)) for s, o in SHAPES]
BWD_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[5]]
BWD_IDS = [IDS[0], IDS[1], IDS[5]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _place(x, dtype, odd, dev):
    """x in `dtype` on the device; odd: as a contiguous view that starts one element (2 bytes) into its storage."""
    x = x.to(dtype)
    if not odd:
        return x.to(dev)
    buf = torch.zeros(x.numel() + 1, dtype=dtype, device=dev)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 8 == 2
    return view


def _volume(seed, shape, dtype, hard):
    """Seeded normal logits scaled by 8; hard: + one column of all-equal values, two planes at -inf, one NaN, the extremes of
    the element type."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 8.0
    if hard:
        big = 65504.0 if dtype == torch.float16 else 1.0e38
        x[:, 1] = -float("inf")
        x[:, D - 2] = -float("inf")
        x[0, :, 1, 2] = 1.25             # an all-equal column
        x[0, 3, 2, 1] = float("nan")
        x[0, 0, 0, 0], x[0, 2, 0, 3] = big, -big
        x[B - 1, 4, H - 1, W - 1], x[B - 1, 5, H - 1, W - 2] = big, big
    return x


_cache = {}


def _case(dtype, shape, odd, dev):
    """Inputs and the fp32 reference of one case, computed once: logits x, addend a (both hard), candidates, and the outputs of
    the fp32 op on the widened inputs, without and with the addend."""
    key = (dtype, shape, odd)
    if key not in _cache:
        B, D, H, W = shape
        x = _place(_volume(11, shape, dtype, True), dtype, odd, dev)
        a = _place(_volume(12, shape, dtype, False), dtype, odd, dev)
        dc = torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0)).float().to(dev)
        kw = dict(want_logp=True, want_prob=True, want_depth=True, want_var=True, want_quarter=True)
        with torch.no_grad():
            ref = ops.dpv_reduce_ex(x.float(), dc, **kw)
            ref_add = ops.dpv_reduce_ex(x.float(), dc, addend=a.float(), **kw)
        _cache[key] = (x, a, dc, kw, ref, ref_add)
    return _cache[key]


def _same_bits(got, want):
    """Equal bit for bit, NaN matching NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bits = torch.int32 if got.dtype == torch.float32 else torch.int16
    same = (got.contiguous().view(bits) == want.contiguous().view(bits)) | (got.isnan() & want.isnan())
    return bool(same.all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape,odd", SHAPES, ids=IDS)
def test_forward_has_the_bits_of_the_fp32_kernel_on_the_widened_input(dev, dtype, shape, odd):
    x, a, dc, kw, ref, ref_add = _case(dtype, shape, odd, dev)
    with torch.no_grad():
        got = ops.dpv_reduce_ex(x, dc, **kw)
        got_add = ops.dpv_reduce_ex(x, dc, addend=a, **kw)
        got_lp = ops.dpv_reduce_ex(x, dc, addend=a, want_logp=False, want_prob=True, prob_dtype=dtype)
        lp, dep = ops.dpv_reduce(x, dc)
        lp32, dep32 = ops.dpv_reduce(x.float(), dc)
        lp_in, _ = ops.dpv_reduce(x, dc, want_depth=False, inplace=True)   # (ignored: the output is another type)
    assert sorted(got) == sorted(got_add) == ["depth", "logp", "prob", "quarter", "var"]
    assert ref["logp"].isnan().any() and torch.isfinite(ref["depth"]).any()   # (the NaN column is there, and is not everything)
    for k in got:
        assert got[k].dtype == torch.float32
        assert _same_bits(got[k], ref[k]), k
        assert _same_bits(got_add[k], ref_add[k]), k + " (addend)"
    assert list(got_lp) == ["prob"] and got_lp["prob"].dtype == dtype
    assert _same_bits(got_lp["prob"], ref_add["prob"].to(dtype))
    assert _same_bits(lp, lp32) and _same_bits(dep, dep32)
    assert lp_in.dtype == torch.float32 and _same_bits(lp_in, lp32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape,odd", [SHAPES[0], SHAPES[3]], ids=[IDS[0], IDS[3]])
def test_forward_against_float64(dev, dtype, shape, odd):
    B, D, H, W = shape
    x = _volume(13, shape, dtype, False).to(dtype)
    dc = synth.powerf(5.0, 40.0, D, 1.0)
    out = ops.dpv_reduce_ex(x.to(dev), dc, want_logp=True, want_depth=True)
    want_lp = torch.log_softmax(x.double(), 1)
    want_d = (torch.exp(want_lp) * torch.from_numpy(dc).view(1, D, 1, 1)).sum(1)
    np.testing.assert_allclose(out["logp"].cpu().numpy(), want_lp.numpy(), rtol=1e-6, atol=3e-6)
    assert (out["depth"].cpu().double() - want_d).abs().max().item() <= DEPTH_ATOL
    assert (torch.exp(out["logp"]).sum(1) - 1).abs().max().item() < 1e-5


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("which", ["g_logp", "g_depth", "g_prob", "all"])
@pytest.mark.parametrize("shape,odd", BWD_SHAPES, ids=BWD_IDS)
def test_backward_is_the_fp32_backward_rounded_once(dev, dtype, shape, odd, which):
    x, a, dc, kw, ref, ref_add = _case(dtype, shape, odd, dev)
    B, D, H, W = shape
    g = torch.Generator().manual_seed(21)
    gs = {"g_logp": torch.randn(shape, generator=g).to(dev), "g_prob": torch.randn(shape, generator=g).to(dtype).to(dev),
          "g_depth": torch.randn((B, H, W), generator=g).to(dev)}
    if which != "all":
        gs = {which: gs[which]}
    logp = ref_add["logp"]
    got = _native.dpv_reduce_backward_lp(logp, dc, dtype, **gs)
    want = _native.dpv_reduce_backward(logp, dc, **{k: v.float() for k, v in gs.items()})
    assert got.dtype == dtype and want.dtype == torch.float32
    assert want.isnan().any() and torch.isfinite(want).any()
    assert _same_bits(got, want.to(dtype))
    if "g_prob" in gs:   # ... and an fp32 g_prob beside half logits (prob was asked for in fp32)
        gs["g_prob"] = gs["g_prob"].float()
        assert _same_bits(_native.dpv_reduce_backward_lp(logp, dc, dtype, **gs), want.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape,odd", BWD_SHAPES, ids=BWD_IDS)
def test_autograd_returns_gradients_in_the_inputs_dtype(dev, dtype, shape, odd):
    x, a, dc, kw, ref, ref_add = _case(dtype, shape, odd, dev)
    B, D, H, W = shape
    g = torch.Generator().manual_seed(31)
    w1 = torch.randn(shape, generator=g).to(dev)
    w2 = torch.randn(shape, generator=g).to(dtype).float().to(dev)   # (a half value: the cast's backward rounds g_prob to the half type)
    w3 = torch.randn((B, H, W), generator=g).to(dev)

    def grads(xx, aa, prob_dtype):
        xx, aa = xx.detach().clone().requires_grad_(), aa.detach().clone().requires_grad_()
        out = ops.dpv_reduce_ex(xx, dc, addend=aa, want_prob=True, prob_dtype=prob_dtype, want_depth=True)
        assert out["prob"].dtype == (prob_dtype or torch.float32) and out["logp"].dtype == out["depth"].dtype == torch.float32
        ((out["logp"] * w1).sum() + (out["prob"].float() * w2).sum() + (out["depth"] * w3).sum()).backward()
        return xx.grad, aa.grad

    gx, ga = grads(x, a, dtype)
    gx32, ga32 = grads(x.float(), a.float(), None)
    assert gx.dtype == ga.dtype == dtype and gx32.dtype == torch.float32
    assert torch.isfinite(gx32).any()
    assert _same_bits(gx, gx32.to(dtype)) and _same_bits(ga, ga32.to(dtype))


def test_errors_name_the_dtypes(dev):
    x = torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16, device=dev)
    dc = torch.linspace(5, 40, 8, device=dev)
    for a in (x.float(), x.half()):
        with pytest.raises(RuntimeError, match=r"torch\.%s.*torch\.bfloat16" % str(a.dtype).split(".")[1]):
            ops.dpv_reduce_ex(x, dc, addend=a)
    with pytest.raises(RuntimeError, match=r"torch\.bfloat16.*torch\.float32"):
        ops.dpv_reduce_ex(x.float(), dc, addend=x)
    for bad in (torch.float16, torch.float64):
        with pytest.raises(RuntimeError, match="prob_dtype"):
            ops.dpv_reduce_ex(x, dc, want_prob=True, prob_dtype=bad)
    with pytest.raises(RuntimeError, match="prob_dtype"):
        ops.dpv_reduce_ex(x.float(), dc, want_prob=True, prob_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.dpv_reduce_ex(x.double(), dc)
    with pytest.raises(RuntimeError, match="expected float32"):
        ops.dpv_reduce(x.double(), dc)
