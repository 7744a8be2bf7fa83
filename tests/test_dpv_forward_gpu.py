"""The forward of the DPV reductions (csrc/dpv.hip, csrc/dpv_reduce_body.hpp, csrc/dpv_moments.hip, csrc/dpv_half.hip) against the
float64 restatement of tests/util_dpv_forward.py: every plane of every pixel inside the a-priori per-element bound derived
there, on every shape of its table (each reaches the kernel the table names) and every column kind -- peaked, tied, flat, offset
by +-1e4, a third of the planes at -inf, one-hot -- for ops.dpv_reduce (plain and in place), ops.dpv_reduce_ex (all outputs at
once and each alone, with and without an addend), ops.dpv_expect and ops.dpv_moments (log and linear volume); non-finite
reference values by pattern and equality, the exact expectations bit for bit; non-finite columns stay in their pixel; the
fp16 / bf16 entries inside the bound of the widened input, prob in the half type with one more rounding.

test_dpv_forward_host.py shows a float32 emulation of both kernel orders inside the bound (logp 0.973, prob 0.947, depth 0.422,
variance 0.300 of it at the worst) and six planted mistakes at least 1.0e3 times outside.

Measured on an MI355X (printed by the tests, -s), worst err / bound over all shapes and kinds, and the kind that gives it:
  dpv_reduce, plain = in place     logp 0.964 (randn30, 1x128x4x68), depth 0.413 (randn30, 2x32x1x257)
  dpv_reduce_ex                    logp 0.964, prob 0.941, quarter 0.948, depth 0.413 (all randn30), var 0.275 (randn30, 2x3x4x4)
  dpv_reduce_ex + addend           logp 0.973, prob 0.932, quarter 0.931, depth 0.412 (all randn30), var 0.259 (masked, 2x3x4x4)
                                   (each output alone: the figures of all at once)
  dpv_expect                       log volume 0.543 (offset), linear 0.791 (randn30, 1x1x1x1: one product, u |d v| is the bound)
  dpv_moments                      log: mean 0.542 (randn30), var 0.292 (masked); linear: mean 0.791 (randn30), var 0.487 (randn0.1)
  fp16 / bf16 logits               logp 0.890 / 0.579, prob 0.775 / 0.569, depth 0.374 / 0.368, var 0.302 / 0.299;
                                   prob in the half type 0.999 / 0.996 (the one rounding of the type is nearly all of that bound)
By kernel (logp / depth of dpv_reduce): scalar 0.96 / 0.41, vec4<8> 0.95 / 0.34, vec4<16> 0.95 / 0.39, vec4<32> 0.96 / 0.32; the
per-pixel extended kernel 0.96 / 0.41 (1x40x4x6: 0.85 / 0.27 against the wave layout's 0.84 / 0.23 on the same input).
randn30 gives the worst ratio of every output of the reductions: there |x_k - m| and |logp_k| reach 150 and their two roundings,
u (|a_k| + |lp_k|), are nearly all of the bound and nearly attained.  The kernels sit where the emulation of their order sits
(the host's 0.973 is the MI355X's 0.973); no defect was found.
With two mistakes planted in a scratch build -- x - (m + ls) in dpv_reduce_scalar_kernel, absent planes filled with 0 in
dpv_reduce_lanes -- test_forward_against_float64 fails on 11 of 14 shapes (170 ... 2400 times the bound on the offset kinds,
the one-hot columns no longer exact; D = 1, 64 and 128 in the wave layout have no absent plane) and the half test on 4 of 6.
"""
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops
import util_dpv_forward as U

pytestmark = pytest.mark.gpu

IDX = list(range(len(U.CASES)))
ALL = dict(want_logp=True, want_prob=True, want_depth=True, want_var=True, want_quarter=True)
ALONE = tuple({"want_" + k: k == name for k in ("logp", "prob", "depth", "var", "quarter")} for name in ("logp", "prob", "depth", "var", "quarter"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _place(t, dev, off=False):
    """A contiguous copy of the host tensor on the device, on a 16-byte boundary or (off) 4 bytes past one."""
    if not off:
        v = t.to(dev).contiguous()
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class _Worst:
    """Worst err / bound per (op, output), with the kind that gave it."""

    def __init__(self):
        self.top = {}

    def note(self, op, checked, kind):
        for name, w in checked.items():
            if w > self.top.get((op, name), (-1.0, None))[0]:
                self.top[(op, name)] = (w, kind)

    def report(self, tag):
        for (op, name), (w, kind) in sorted(self.top.items()):
            print("%s: %-28s %-7s worst err / bound = %.3f (%s)" % (tag, op, name, w, kind))
        over = {k: v for k, v in self.top.items() if not v[0] <= 1.0}
        assert not over, (tag, over)


# ---- every shape, every kind, every op ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", IDX, ids=U.CASE_IDS)
def test_forward_against_float64(dev, idx):
    shape, off, ipa = U.CASES[idx]
    D = shape[1]
    dc_host = U.candidates(idx)
    dc = dc_host.to(dev)
    a = U.addend(idx).to(dev)
    aligned = not off
    worst = _Worst()
    for kind in U.kinds_for(D):
        x_host = U.logits(idx, kind)
        x = _place(x_host, dev, off)
        keep = x.clone()
        # dpv_reduce, plain and in place
        r = U.reference(idx, kind)
        E = U.bound(idx, kind, False, U.order_of("reduce", shape, aligned))
        for inplace in (False, True):
            xin = _place(x_host, dev, off) if inplace else x
            lp, dep = ops.dpv_reduce(xin, dc, inplace=inplace)
            assert (lp.data_ptr() == xin.data_ptr()) == inplace
            out = {"logp": lp, "depth": dep}
            worst.note("dpv_reduce" + (" in place" if inplace else ""), U.check_outputs(out, r["f"], E), kind)
            assert U.exact_failures(x_host, dc_host, out) == 0, (kind, inplace)
        # dpv_reduce_ex: all outputs and each alone, without and with the addend; in place where the case says so
        for with_addend in (False, True):
            r = U.reference(idx, kind, with_addend)
            for wants in (ALL,) + ALONE:
                if wants is ALONE[4] and (shape[2] < 4 or shape[3] < 4):
                    continue   # an empty quarter alone is no output at all: the entry refuses the call
                # (in place = logp written over the logits: without the logp output nothing is in place)
                E = U.bound(idx, kind, with_addend, U.order_of("reduce_ex", shape, aligned,
                                                              inplace_addend=ipa and with_addend and wants["want_logp"]))
                xin = _place(x_host, dev, off) if ipa else x
                out = ops.dpv_reduce_ex(xin, dc, addend=a if with_addend else None, inplace=ipa, **wants)
                assert sorted(out) == sorted(k[5:] for k, on in wants.items() if on)
                if ipa and wants["want_logp"]:
                    assert out["logp"].data_ptr() == xin.data_ptr()
                op = "dpv_reduce_ex%s%s" % (" + addend" if with_addend else "", "" if wants is ALL else " alone")
                worst.note(op, U.check_outputs(out, r["f"], E), kind)
                assert U.exact_failures(r["x32"], dc_host, out) == 0, (kind, with_addend, wants)
        assert torch.equal(x, keep)   # only an in-place call writes its input
        # dpv_expect and dpv_moments of a given volume, log and linear
        for bv_log in (True, False):
            v = U.volume_reference(idx, kind, bv_log)
            vol = _place(U.volume(idx, kind, bv_log), dev, off)
            form = "log" if bv_log else "linear"
            E = U.volume_bound(v, U.order_of("expect", shape, aligned))
            worst.note("dpv_expect " + form, {"depth": U.worst(ops.dpv_expect(vol, dc, BV_log=bv_log), v["depth"], E["depth"])}, kind)
            E = U.volume_bound(v, U.order_of("moments", shape))
            mean, var = ops.dpv_moments(vol, dc, BV_log=bv_log)
            worst.note("dpv_moments " + form, {"depth": U.worst(mean, v["depth"], E["depth"]), "var": U.worst(var, v["var"], E["var"])}, kind)
    worst.report(U.CASE_IDS[idx])


# ---- non-finite columns ----------------------------------------------------------------------------------------------------
def _assert_contained(got, clean, mask, tag):
    """Every element of a pixel of `mask` is NaN; every other pixel has the bits of the clean run."""
    for k in got:
        g, c = got[k].cpu(), clean[k].cpu()
        if k == "quarter":
            H, W = mask.shape[1:]
            m = mask[:, ::4, ::4][:, :H // 4, :W // 4]
        else:
            m = mask
        m = m.unsqueeze(1).expand_as(g) if g.dim() == 4 else m
        assert bool(g[m].isnan().all()), (tag, k)
        assert torch.equal(g[~m], c[~m]) and bool(torch.isfinite(c[~m]).all()), (tag, k)


@pytest.mark.parametrize("what", U.PLANTS)
@pytest.mark.parametrize("idx", U.NONFINITE_CASES, ids=[U.CASE_IDS[i] for i in U.NONFINITE_CASES])
def test_non_finite_columns_stay_in_their_pixel(dev, idx, what):
    shape = U.SHAPES[idx]
    dc_host = U.candidates(idx)
    dc = dc_host.to(dev)
    x_host = U.logits(idx, "randn3")
    bad_host, mask = U.plant(x_host, shape, what)
    assert int(mask.sum()) == len(U.nonfinite_pixels(shape)) >= 6
    # the reference agrees: float64 log_softmax is NaN on every plane of those pixels and finite elsewhere
    want = torch.log_softmax(bad_host.double(), 1)
    assert bool(want[mask.unsqueeze(1).expand_as(want)].isnan().all()) and bool(torch.isfinite(want[~mask.unsqueeze(1).expand_as(want)]).all())
    x, bad, a = x_host.to(dev), bad_host.to(dev), U.addend(idx).to(dev)
    for addend in (None, a):
        _assert_contained(ops.dpv_reduce_ex(bad, dc, addend=addend, **ALL), ops.dpv_reduce_ex(x, dc, addend=addend, **ALL), mask,
                          (what, addend is not None))
    for inplace in (False, True):
        got, clean = ops.dpv_reduce(bad.clone(), dc, inplace=inplace), ops.dpv_reduce(x.clone(), dc, inplace=inplace)
        _assert_contained({"logp": got[0], "depth": got[1]}, {"logp": clean[0], "depth": clean[1]}, mask, (what, "reduce", inplace))
    # a given volume: exp(+inf) = inf and exp(-inf) = 0 are values, not errors -- the planted pixels follow the float64
    # restatement's pattern (NaN, inf or the exact 0), every other pixel keeps its bits
    for bv_log in (True, False):
        vol_host = U.volume(idx, "randn3", bv_log)
        badv_host, _ = U.plant(vol_host, shape, what)
        v = U.volume64(badv_host, dc_host, bv_log)
        E = U.volume_bound(v, U.ASCENDING)
        vol, badv = vol_host.to(dev), badv_host.to(dev)
        mean, var = ops.dpv_moments(badv, dc, BV_log=bv_log)
        exp = ops.dpv_expect(badv, dc, BV_log=bv_log)
        clean_mean, clean_var = ops.dpv_moments(vol, dc, BV_log=bv_log)
        clean_exp = ops.dpv_expect(vol, dc, BV_log=bv_log)
        for got, clean, name in ((mean, clean_mean, "depth"), (var, clean_var, "var"), (exp, clean_exp, "depth")):
            assert torch.equal(got.cpu()[~mask], clean.cpu()[~mask]), (what, bv_log, name)
            fin = torch.isfinite(v[name])
            r = U.ratio(got, v[name], E[name])
            assert bool((r[mask & ~fin] == 0).all()), (what, bv_log, name)        # the pattern
            if what == "minus_inf_column" and bv_log:                             # exp(-inf) = 0 on every plane: an exact 0
                assert bool((got.cpu()[mask] == 0).all()), (what, name)


# ---- fp16 / bf16 logits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("idx", U.HALF_CASES, ids=[U.CASE_IDS[i] for i in U.HALF_CASES])
def test_half_entries_against_float64_of_the_widened_input(dev, idx, dtype):
    shape = U.SHAPES[idx]
    dc_host = U.candidates(idx)
    dc = dc_host.to(dev)
    order = U.order_of("reduce_ex", shape, half=True)
    ah = U.addend(idx).to(dtype)
    worst = _Worst()
    for kind in U.kinds_for(shape[1]):
        xh = U.logits(idx, kind).to(dtype)
        for with_addend in (False, True):
            wide = xh.float() + ah.float() if with_addend else xh.float()   # widening is exact; the sum is one float32 rounding
            f = U.forward64(wide, dc_host)
            E = U.forward_bound(f, order)
            add = ah.to(dev) if with_addend else None
            out = ops.dpv_reduce_ex(xh.to(dev), dc, addend=add, **ALL)
            assert all(t.dtype == torch.float32 for t in out.values())
            tag = "half dpv_reduce_ex" + (" + addend" if with_addend else "")
            worst.note(tag, U.check_outputs(out, f, E), kind)
            assert U.exact_failures(wide, dc_host, out) == 0, (kind, with_addend)
            low = ops.dpv_reduce_ex(xh.to(dev), dc, addend=add, want_logp=False, want_prob=True, prob_dtype=dtype)["prob"]
            assert low.dtype == dtype
            worst.note(tag + ", prob in the half type", {"prob": U.worst(low.float(), f["prob"], U.half_rounding(f["prob"], E["prob"], dtype))}, kind)
            assert torch.equal(low, out["prob"].to(dtype))   # exactly one more rounding, of the float32 prob
        lp, dep = ops.dpv_reduce(xh.to(dev), dc)
        f = U.forward64(xh.float(), dc_host)
        worst.note("half dpv_reduce", U.check_outputs({"logp": lp, "depth": dep}, f, U.forward_bound(f, order)), kind)
    worst.report("%s %s" % (U.CASE_IDS[idx], str(dtype).split(".")[1]))
