"""GPU suite of the deterministic scattered gradients (csrc/sweep_bwd_det.hip, csrc/scatter_det.hip; the `deterministic`
keyword of ops.sweep_cost / sweep_dpv / depth_stereo_consistency, utils.inverse_warp under torch.use_deterministic_algorithms).

The contributions of the integer sum are those of the float-atomic kernels bit for bit, so accuracy is held to the bounds the
atomic paths are held to, against the same float64 references on the same inputs (tests/test_sweep_backward_groups.py,
tests/test_sweep_backward.py, tests/test_loss_terms_gpu.py, tests/test_warps_gpu.py; the references are computed once and shared
with those suites).  What is new is the structure: the same bits from call to call, whatever else is requested, wherever an item
or a view stands in the batch, whatever the magnitudes of the other items; exact zeros; a non-finite input turns its own item
NaN and leaves the others' bits alone; no host synchronisation."""
import copy

import pytest
import torch
import torch.nn.functional as F

import pdepth_amd  # noqa: F401
from pdepth_amd import ops, synth
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.utils import inverse_warp as iv
import test_loss_terms_gpu as TL
import test_sweep_backward_groups as G
import test_sweep_backward_pin_gpu as P
import test_warps_gpu as TW
import util_loss_terms as LT
import util_warps as UW
from util_sweep_backward import l1_allowance, oracle_grads, pin_check, rel_err, to_dev

pytestmark = pytest.mark.gpu
SIGMA = G.SIGMA
TOL = 1e-4          # rel_err of a gradient against float64 (tests/test_sweep_backward.py, tests/test_sweep_backward_groups.py)
NAMES, METRICS = G.NAMES, G.METRICS
_memo = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def det_grads(d, gup, sigma, metric, want_ref=True, want_src=True, deterministic=True):
    """util_sweep_backward.hip_grads with the keyword: (g_ref, g_src) of ops.sweep_cost."""
    ref = d["ref"].clone().requires_grad_(want_ref)
    src = d["src"].clone().requires_grad_(want_src)
    kw = {} if deterministic is None else {"deterministic": deterministic}
    cost = ops.sweep_cost(ref, src, d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], sigma, feat_dist=metric, **kw)
    (cost * gup).sum().backward()
    return ref.grad, src.grad


def _det(dev, name, metric):
    """(g_ref, g_src) of the deterministic both-outputs call on a group case, once."""
    key = ("det", name, metric)
    if key not in _memo:
        r = G._result(dev, name, metric)
        _memo[key] = det_grads(r["d"], r["gup"], SIGMA, metric)
    return _memo[key]


# ---- sweep: against float64 ------------------------------------------------------------------------------------------------
def _assert_src(tag, gs, gs_atomic, s64, allow):
    """g_src, and each view against its own maximum, within TOL of float64; the atomic path's figures beside it."""
    def errs(g):
        out = [rel_err(g, s64, allow)]
        for v in range(g.shape[1]):
            out.append(rel_err(g[:, v], s64[:, v], None if allow is None else allow[:, v]))
        return out
    e_det, e_atomic = errs(gs), errs(gs_atomic)
    print("%s rel_err [g_src, per view ...]: deterministic %s, atomic %s" % (tag, ["%.2e" % e for e in e_det], ["%.2e" % e for e in e_atomic]))
    for i, e in enumerate(e_det):
        assert e <= TOL, (tag, "g_src" if i == 0 else "view %d against its own max" % (i - 1), e)
    if allow is not None:   # the allowance is the exception, not the rule
        touched = int((allow > 0).sum()) / allow.numel()
        assert touched <= 1e-2, touched


def _assert_pinned(tag, x, gr, gs, gs_atomic):
    """The same gradients under the per-element bound of tests/util_sweep_backward.py (float64 at the kernel's own positions; the
    integer sum with its quantisation term), on the same input: x is the reference of tests/test_sweep_backward_pin_gpu.py."""
    pin_check(gr, x, "ref", tag + " g_ref")
    pin_check(gs_atomic, x, "src", tag + " g_src atomic")
    pin_check(gs, x, "src", tag + " g_src deterministic", det=True)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_sweep_group_cases_against_float64(dev, name, metric):
    """Split groups, direct planes, empty runs, the channel tail (test_cases_reach_the_split_direct_and_empty_paths)."""
    r = G._result(dev, name, metric)
    gr, gs = _det(dev, name, metric)
    assert torch.equal(gr, r["gr"])   # g_ref is the gather pass either way
    _assert_src("%s %s" % (name, metric), gs, r["gs"], r["s64"], r["as_"])
    _assert_pinned("%s %s" % (name, metric), P.reference(name, metric), gr, gs, r["gs"])


@pytest.mark.parametrize("metric,V,C,D,pose", [("L2", 2, 67, 64, "stereo"), ("L1", 4, 80, 128, "wide")])
def test_sweep_ordinary_cases_against_float64(dev, metric, V, C, D, pose):
    b = synth.make_batch(23, 2, C=C, D=D, H=24, W=40, V=V, pose=pose, cx_off=0.0)
    gup = torch.randn(2, D, 24, 40, generator=torch.Generator().manual_seed(5)).to(dev)
    r64, s64 = oracle_grads(b, gup, SIGMA, metric, torch.float64, dev)
    ar, as_ = l1_allowance(b, gup, SIGMA, dev) if metric == "L1" else (None, None)
    d = to_dev(b, dev)
    gr_a, gs_a = det_grads(d, gup, SIGMA, metric, deterministic=False)
    gr, gs = det_grads(d, gup, SIGMA, metric)
    assert torch.equal(gr, gr_a) and rel_err(gr, r64, ar) <= TOL
    _assert_src("%s V=%d C=%d D=%d %s" % (metric, V, C, D, pose), gs, gs_a, s64, as_)
    _assert_pinned("%s V=%d C=%d D=%d %s" % (metric, V, C, D, pose), P.reference("ordinary-%d-%d-%d-%s-0.0" % (V, C, D, pose), metric), gr, gs, gs_a)


# ---- sweep: the same bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_sweep_same_bits_across_calls_and_requests(dev, name, metric):
    r = G._result(dev, name, metric)
    gr, gs = _det(dev, name, metric)
    assert bool(torch.isfinite(gs).all()) and float(gs.abs().max()) > 0
    for _ in range(2):   # three consecutive calls in all
        gr2, gs2 = det_grads(r["d"], r["gup"], SIGMA, metric)
        assert torch.equal(gs2, gs) and torch.equal(gr2, gr)
    none, only = det_grads(r["d"], r["gup"], SIGMA, metric, want_ref=False)   # without g_ref requested
    assert none is None and torch.equal(only, gs)
    gr3, none = det_grads(r["d"], r["gup"], SIGMA, metric, want_src=False)
    assert none is None and torch.equal(gr3, r["gr"])


@pytest.mark.parametrize("metric", METRICS)
def test_sweep_does_not_depend_on_the_order_of_items_or_views(dev, metric):
    """Case R (B = 2, V = 2).  What a scale per call instead of per item would break: the items' maxima differ."""
    r = G._result(dev, "R", metric)
    _, gs = _det(dev, "R", metric)
    d, gup = r["d"], r["gup"]
    assert d["src"].shape[:2] == (2, 2)
    items = dict(d, **{k: d[k].flip(0).contiguous() for k in ("ref", "src", "K", "R", "t", "rays", "cxcy")})
    _, swapped = det_grads(items, gup.flip(0).contiguous(), SIGMA, metric)
    assert torch.equal(swapped, gs.flip(0))
    views = dict(d, **{k: d[k].flip(1).contiguous() for k in ("src", "R", "t")})
    _, swapped = det_grads(views, gup, SIGMA, metric)
    assert torch.equal(swapped, gs.flip(1))


@pytest.mark.parametrize("metric", METRICS)
def test_sweep_dynamic_range_per_item(dev, metric):
    """g_cost[0] x 1e-25 and g_cost[1] x 1e+25 in one call: each item within TOL of float64 relative to ITS OWN maximum (the
    gradient is linear in g_cost: the float64 reference is scaled).  Then g_cost[0] = 0: that item is exactly zero."""
    r = G._result(dev, "R", metric)
    f = torch.tensor([1e-25, 1e25], dtype=torch.float64, device=dev)
    gup = (r["gup"].double() * f.view(2, 1, 1, 1)).float()
    _, gs = det_grads(r["d"], gup, SIGMA, metric)
    _, gs_a = det_grads(r["d"], gup, SIGMA, metric, deterministic=False)
    assert bool(torch.isfinite(gs).all())
    for i in range(2):
        want = r["s64"][i] * f[i]
        allow = None if r["as_"] is None else r["as_"][i] * f[i]
        e, e_a = rel_err(gs[i], want, allow), rel_err(gs_a[i], want, allow)
        print("R %s item %d (g_cost x %g): rel_err deterministic %.2e, atomic %.2e" % (metric, i, float(f[i]), e, e_a))
        assert e <= TOL, (i, e)
    gup0 = r["gup"].clone()
    gup0[0] = 0
    _, gz = det_grads(r["d"], gup0, SIGMA, metric)
    assert int(torch.count_nonzero(gz[0])) == 0 and not bool(torch.isnan(gz[0]).any())
    _, gs_clean = _det(dev, "R", metric)
    assert torch.equal(gz[1], gs_clean[1])   # ... and its neighbour has the bits of the ordinary call


def test_sweep_non_finite_input_turns_its_own_item_nan(dev):
    r = G._result(dev, "R", "L2")
    _, clean = _det(dev, "R", "L2")
    gup = r["gup"].clone()
    gup[1, 3, 17, 29] = float("nan")
    _, gs = det_grads(r["d"], gup, SIGMA, "L2")
    assert torch.equal(gs[0], clean[0]) and bool(torch.isnan(gs[1]).all())
    d = dict(r["d"], src=r["d"]["src"].clone())
    d["src"][1, 0, 2, 11, 13] = float("inf")
    _, gs = det_grads(d, r["gup"], SIGMA, "L2")
    assert torch.equal(gs[0], clean[0]) and bool(torch.isnan(gs[1]).all())


# ---- sweep: the switch, the fused op, no synchronisation ---------------------------------------------------------------------
def test_sweep_follows_the_deterministic_switch(dev):
    r = G._result(dev, "A", "L2")
    _, gs = _det(dev, "A", "L2")
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        _, by_switch = det_grads(r["d"], r["gup"], SIGMA, "L2", deterministic=None)
        _, forced_off = det_grads(r["d"], r["gup"], SIGMA, "L2", deterministic=False)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.equal(by_switch, gs)
    assert rel_err(forced_off, r["s64"]) <= TOL   # the atomic path still runs under the switch
    _, default_off = det_grads(r["d"], r["gup"], SIGMA, "L2", deterministic=None)   # switch off, no keyword: today's path
    assert rel_err(default_off, r["s64"]) <= TOL


def test_sweep_dpv_deterministic_gradients(dev):
    """ops.sweep_dpv with logp and depth gradients against the sweep_cost + torch-tail chain, to the tolerance of
    tests/test_sweep_backward.py::test_sweep_dpv_gradients_in_any_combination; two calls carry the same bits."""
    d = to_dev(synth.make_batch(24, 2, C=67, D=64, H=32, W=48, V=2, pose="mono"), dev)
    gen = torch.Generator().manual_seed(7)
    _, gl, gd = (torch.randn(2, 64, 32, 48, generator=gen).to(dev), torch.randn(2, 64, 32, 48, generator=gen).to(dev),
                 torch.randn(2, 32, 48, generator=gen).to(dev))
    args = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    grads = []
    for _ in range(2):
        ref, src = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
        _, logp, depth = ops.sweep_dpv(ref, src, *args, want_cost=False, want_logp=True, want_depth=True, deterministic=True)
        ((logp * gl).sum() + (depth * gd).sum()).backward()
        grads.append((ref.grad, src.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    ref2, src2 = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
    cost = ops.sweep_cost(ref2, src2, *args, deterministic=True)
    logp = F.log_softmax(cost, dim=1)
    depth = (torch.exp(logp) * ops.d_candi_tensor(d["d_candi"], dev).view(1, -1, 1, 1)).sum(1)
    ((logp * gl).sum() + (depth * gd).sum()).backward()
    for a, b_ in ((grads[0][0], ref2.grad), (grads[0][1], src2.grad)):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-5 * float(b_.abs().max()))


def test_sweep_deterministic_backward_does_not_synchronise(dev):
    r = G._result(dev, "A", "L2")
    _, gs = _det(dev, "A", "L2")   # (first call done: the depth candidates are on the device)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, again = det_grads(r["d"], r["gup"], SIGMA, "L2")
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(again, gs)


# ---- depth stereo consistency ----------------------------------------------------------------------------------------------
def _dsc_kernel(deterministic):
    def fn(term, t, x):
        return ops.depth_stereo_consistency(x["src_depth"], x["tgt_depth"], t["src_mask"], t["Kinv"], t["proj"], t["back"][:, 2], t["intr"],
                                            deterministic=deterministic)
    return fn


def _assert_dsc(tag, g_det, g_comp, g64):
    """The criterion of test_loss_terms_gpu.py::test_against_float64 for a gradient: 2 max E_ref + 1e-6 of the largest gradient."""
    for n in g64:
        k, c, r = g_det[n].double().cpu(), g_comp[n].double().cpu(), g64[n]
        ek, er, big = float((k - r).abs().max()), float((c - r).abs().max()), float(r.abs().max())
        print(tag, "gradient", n, "deterministic max error %.3e  E_ref max %.3e  largest gradient %.3e" % (ek, er, big))
        assert bool(torch.isfinite(r).all()) and big > 0
        assert ek <= 2 * er + 1e-6 * big, (tag, n, ek, er, big)


@pytest.mark.parametrize("shape", LT.SHAPES)
def test_dsc_against_float64_and_same_bits(dev, shape):
    _, t = TL._inputs(shape)
    _, g64 = TL._reference("dsc", shape)
    v_det, g_det = TL._run(_dsc_kernel(True), "dsc", t)
    v_at, g_at = TL._run(_dsc_kernel(False), "dsc", t)
    _, g_comp = TL._run(TL._composition, "dsc", t)
    _assert_dsc("dsc %s" % (shape,), g_det, g_comp, g64)
    assert torch.equal(v_det, v_at)                                # the forward is untouched
    assert torch.equal(g_det["tgt_depth"], g_at["tgt_depth"])      # written per owner: the atomic path's bits
    for _ in range(2):
        _, again = TL._run(_dsc_kernel(True), "dsc", t)
        assert torch.equal(again["src_depth"], g_det["src_depth"]) and torch.equal(again["tgt_depth"], g_det["tgt_depth"])


def _eighth(proj):
    """The projection with focal lengths (and principal point) an eighth of the intrinsics': a 32 x 48 image lands on about
    4 x 6 texels, some fifty contributions each -- the order of the adds matters."""
    s = torch.tensor([0.125, 0.125, 1.0], dtype=proj.dtype, device=proj.device).view(1, 3, 1)
    return (proj * s).contiguous()


def _dsc_composition_with_matrices(term, t, x):
    """losses/loss_blocks.py depth_stereo_consistency_loss(per_item=True) with the warp's two matrices given (float32, device)."""
    B, H, W = x["tgt_depth"].shape
    moved = iv.transform_dmap(x["src_depth"], t["back"], t["intr"])
    moved = (moved * t["src_mask"].float().reshape(B, H, W)).unsqueeze(1)
    warped, valid = iv.warp_with_matrices(moved, x["tgt_depth"], t["Kinv"], t["proj"], "nearest")
    mask = ((valid & lb._lower_two_thirds(valid.shape, valid.device)).unsqueeze(1) & (warped > 0.)).float()
    tgt = (x["tgt_depth"].unsqueeze(1) * mask).clamp(min=1e-3)
    got = (warped * mask).clamp(min=1e-3)
    diff = ((tgt - got).abs() / (tgt + got).abs()).clamp(0, 1)
    return lb.mean_on_mask(diff, mask, True)


def test_dsc_many_to_one(dev):
    shape = (2, 32, 48)
    cpu, t = TL._inputs(shape)
    cpu, t = dict(cpu, proj=_eighth(cpu["proj"])), dict(t, proj=_eighth(t["proj"]))
    _, g64 = TL._run(TL._restatement, "dsc", cpu, torch.float64)
    v_det, g_det = TL._run(_dsc_kernel(True), "dsc", t)
    _, g_comp = TL._run(_dsc_composition_with_matrices, "dsc", t)
    hit = int((g64["src_depth"] != 0).sum())
    print("dsc many-to-one: %d texels of %d receive a gradient" % (hit, g64["src_depth"].numel()))
    assert 0 < hit <= 2 * 8 * 12 and bool(torch.isfinite(v_det).all())
    _assert_dsc("dsc many-to-one", g_det, g_comp, g64)
    for _ in range(2):
        _, again = TL._run(_dsc_kernel(True), "dsc", t)
        assert torch.equal(again["src_depth"], g_det["src_depth"])


# ---- inverse_warp ------------------------------------------------------------------------------------------------------------
class _switch:
    def __enter__(self):
        self.was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(True, warn_only=True)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.was[0], warn_only=self.was[1])
        return False


@pytest.mark.parametrize("name", TW.IW_NAMES)
@pytest.mark.parametrize("mode", UW.MODES)
def test_inverse_warp_against_float64_and_same_bits(dev, name, mode):
    """utils.inverse_warp.inverse_warp under the switch: g_img within the bound of tests/test_warps_gpu.py of float64, the same
    bits in three calls; what is written per owner (out, and g_depth behind grad_point) has the atomic path's bits."""
    c = UW.inverse_warp_case(name)
    ref = UW.inverse_warp_reference(name, mode)
    atomic = TW._hip_cached(name, mode, dev)
    with _switch():
        runs = [TW._hip(c, mode, dev, ref["gup"]) for _ in range(3)]
    got = runs[0]
    want = ref["q"]["g_img"]
    m = UW.element_mask("g_img", ref["M"], want)
    err, bound = UW.masked_err(got["g_img"], want, m), UW.inverse_warp_bound(name, mode, "g_img")
    print("%s/%s g_img: deterministic err %.2e, atomic err %.2e, bound %.2e" % (name, mode, err, UW.masked_err(atomic["g_img"], want, m), bound))
    assert err <= bound
    assert not bool(torch.isnan(got["g_img"]).any())
    for again in runs[1:]:
        assert torch.equal(again["g_img"], got["g_img"])
    assert torch.equal(torch.nan_to_num(got["out"], nan=1e30), torch.nan_to_num(atomic["out"], nan=1e30))
    assert torch.equal(torch.nan_to_num(got["g_depth"], nan=1e30), torch.nan_to_num(atomic["g_depth"], nan=1e30))


def _warp_torch(img, depth, Kinv, proj, mode, dtype):
    """inverse_warp from its two matrices in plain torch on `dtype` (CPU): (out, ix, iy, pz)."""
    B, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(1, 3, H * W)
    cam = torch.matmul(Kinv.to(dtype), pix) * depth.to(dtype).reshape(B, 1, H * W)
    pc = torch.matmul(proj.to(dtype)[:, :, :3], cam) + proj.to(dtype)[:, :, 3:]
    Z = pc[:, 2].clamp(min=1e-3)
    xn, yn = 2 * (pc[:, 0] / Z) / (W - 1) - 1, 2 * (pc[:, 1] / Z) / (H - 1) - 1
    grid = torch.stack([xn, yn], dim=-1).reshape(B, H, W, 2)
    out = F.grid_sample(img, grid, mode=mode, padding_mode="zeros", align_corners=False)
    return out, (((xn + 1) * W - 1) / 2).reshape(B, H, W), (((yn + 1) * H - 1) / 2).reshape(B, H, W), pc[:, 2].reshape(B, H, W)


def _many_to_one_case():
    """A 32 x 48 image projected with an eighth of the focal lengths: (inputs of util_warps, Kinv, proj)."""
    B, C, H, W = 2, 3, 32, 48
    c = UW._iw_inputs(6131, B, C, H, W)
    pose = UW._pose44(B, UW._T3[:2], UW._A3[:2])
    return c, torch.inverse(c["K"].double()).float(), _eighth(torch.matmul(c["K"], pose[:, :3]))


def _many_to_one_g_img(dev, c, Kinv, proj, mode, gup, deterministic):
    img = c["img"].to(dev).requires_grad_(True)
    out, _ = iv.warp_with_matrices(img, c["depth"].to(dev), Kinv.to(dev), proj.to(dev), mode, deterministic=deterministic)
    (out * gup.to(dev)).sum().backward()
    return img.grad.cpu()


@pytest.mark.parametrize("mode", UW.MODES)
def test_inverse_warp_many_to_one(dev, mode):
    """A 32 x 48 image projected with an eighth of the focal lengths: about 4 x 6 texels take every contribution.  g_img against
    float64 under the bound of tests/test_warps_gpu.py -- max(4 e_ref, 4 eps32 max|f64|), e_ref the float32 evaluation of the
    same chain in torch, the upstream gradient zero off util_warps.stable_mask --, and three calls with the same bits."""
    c, Kinv, proj = _many_to_one_case()
    B, C, H, W = c["img"].shape
    img64 = c["img"].double().requires_grad_(True)
    out64, ix, iy, pz = _warp_torch(img64, c["depth"], Kinv, proj, mode, torch.float64)
    M = UW.stable_mask(ix.detach(), iy.detach(), pz.detach(), H, W, mode)
    gup = c["gout"] * M.unsqueeze(1)
    (out64 * gup.double()).sum().backward()
    want = img64.grad
    img32 = c["img"].clone().requires_grad_(True)
    (_warp_torch(img32, c["depth"], Kinv, proj, mode, torch.float32)[0] * gup).sum().backward()
    e_ref, scale = float((img32.grad.double() - want).abs().max()), float(want.abs().max())
    bound = max(4 * e_ref, 4 * UW.EPS32 * scale)
    hit = int((want != 0).any(1).sum())
    assert float(M.double().mean()) > 0.9 and 0 < hit <= B * 8 * 12, (float(M.double().mean()), hit)

    def run(deterministic):
        return _many_to_one_g_img(dev, c, Kinv, proj, mode, gup, deterministic)

    got, atomic = run(True), run(False)
    err = float((got.double() - want).abs().max())
    print("many-to-one/%s g_img: %d texels hit; deterministic err %.2e, atomic err %.2e, e_ref %.2e, bound %.2e"
          % (mode, hit, err, float((atomic.double() - want).abs().max()), e_ref, bound))
    assert err <= bound
    assert torch.equal(run(True), got) and torch.equal(run(True), got)


def test_inverse_warp_many_to_one_atomic_and_deterministic_agree_to_the_bit(dev):
    """Both paths run one scatter body, so where float addition is exact they must agree to the bit: the many-to-one case in
    nearest mode with an upstream gradient of integers in [-8, 8].  Every contribution is then an integer and a texel receives
    at most H W = 1536 of them: |sum| <= 12 288 < 2^24, the float atomic sum is exact in any order and so is the integer sum.
    (No such input exists in bilinear mode: g w is not exactly summable.)"""
    c, Kinv, proj = _many_to_one_case()
    gup = torch.randint(-8, 9, tuple(c["img"].shape), generator=torch.Generator().manual_seed(6131)).float()
    assert bool((gup != 0).any()) and float(gup.abs().max()) <= 8.0
    atomic = _many_to_one_g_img(dev, c, Kinv, proj, "nearest", gup, False)
    det = _many_to_one_g_img(dev, c, Kinv, proj, "nearest", gup, True)
    print("many-to-one/nearest, integer gradient: %d texels non-zero, max |g_img| %.0f" % (int((det != 0).sum()), float(det.abs().max())))
    assert bool((det != 0).any())
    assert torch.equal(atomic, det)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_base_model_sweep_gradient_carries_the_same_bits(dev):
    """BaseModel 'default' with the seeded weights and the loss of tests/test_sweep_backward.py::test_base_model_trains, on a
    256 x 256 image, with sweep_deterministic = True: the gradient arriving at the sweep's src input (hooked) is bit-equal across
    two forward + backward passes.  Nothing is claimed about the convolutions around it: their determinism is PyTorch's / MIOpen's
    to set, and the test sets it (without torch.backends.cudnn.deterministic the hooked gradient differed between two passes on
    an MI355X; with it the sweep's src, cost and incoming g_cost are bit-equal as well, which the test prints)."""
    from pdepth_amd.models.get_model import get_model
    import test_sweep_backward as TS
    cfg = synth.default_cfg("default")
    torch.manual_seed(0)
    model = get_model(cfg, 0)
    synth.seed_weights(model, seed=31)
    model = model.to(dev).train()
    model.sweep_deterministic = True
    inp = to_dev(synth.make_model_input(3100, B=2, V=1, H=256, W=256, D=64, pose="mono"), dev)
    target = torch.rand(2, 256, 256, generator=torch.Generator().manual_seed(2)).to(dev) * 30 + 5
    caught, flags, seen = [], [], []
    real = ops.sweep_cost

    def hooked(ref, src, *a, **k):
        flags.append(k.get("deterministic"))
        assert src.requires_grad
        src.register_hook(lambda g: caught.append(g.detach().clone()))
        cost = real(ref, src, *a, **k)
        seen.append([src.detach().clone(), cost.detach().clone(), None])
        cost.register_hook(lambda g, slot=seen[-1]: slot.__setitem__(2, g.detach().clone()))
        return cost

    # the convolutions around the sweep are the caller's to make reproducible (torch.backends.cudnn.deterministic selects MIOpen's
    # deterministic algorithms); this test is that caller
    was = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    ops.sweep_cost = hooked
    try:
        for m in (model, copy.deepcopy(model)):   # (two copies: a pass may move batch-norm statistics)
            TS._model_loss(m, inp, target).backward()
    finally:
        ops.sweep_cost = real
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was
    assert flags == [True, True] and len(caught) == 2
    assert bool(torch.isfinite(caught[0]).all()) and float(caught[0].abs().max()) > 0
    print("between the two passes: src equal %s, cost equal %s, g_cost equal %s (max |diff| %.3e of %.3e), g_src max |diff| %.3e of %.3e"
          % (torch.equal(seen[0][0], seen[1][0]), torch.equal(seen[0][1], seen[1][1]), torch.equal(seen[0][2], seen[1][2]),
             float((seen[0][2] - seen[1][2]).abs().max()), float(seen[0][2].abs().max()),
             float((caught[0] - caught[1]).abs().max()), float(caught[0].abs().max())))
    assert torch.equal(caught[0], caught[1])
