"""GPU suite of the fused consistency and smoothness terms (csrc/loss_terms.hip; ops.depth_stereo_consistency,
rgb_stereo_consistency, depth_consistency, edge_aware_smoothness; BaseLoss(fused_terms=True)).

Per term and shape of util_loss_terms.SHAPES: the mask count equals the composition's (losses/loss_blocks.py on the same device)
exactly; value and every gradient element are measured against the float64 restatement of util_loss_terms.py next to the float32
composition's own error against it (E_ref): a value may err by 2 E_ref + 4 ulp, a gradient element by 2 max E_ref + 1e-6 of the
tensor's largest gradient (the kernel and the composition differ in summation order and fma contraction only: independent
roundings of equal size, hence the factor two).  No pixel is left out anywhere.  Then structure (bit-identical repeats), the
pinned corners, and BaseLoss with the fused terms against the reference (fixture g24) and against the composition."""
import functools

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
from pdepth_amd.utils import img_utils
from pdepth_amd.utils import inverse_warp as iv
from util import golden
import util_loss as U
import util_loss_terms as LT

pytestmark = pytest.mark.gpu
TERMS = ("dsc", "rsc", "dc", "smooth")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


# ---- the three sides of a term: kernel, composition (float32, same device), restatement (float64, CPU) ---------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """The maker's inputs on the CPU and on the device, with the camera matrices formed on the device as BaseLoss forms them."""
    cpu = LT.make_inputs(*shape)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in cpu.items()}
    d["Kinv"], d["proj"], d["back"] = LT.camera_matrices(d["intr"], cpu["T"], lb._inv3)
    d["pose"] = cpu["T"].unsqueeze(0).cuda()
    for k in ("Kinv", "proj", "back"):
        cpu[k] = d[k].cpu()
    return cpu, d


def _leaves(term, t, dtype=None):
    """The differentiable inputs of a term, as fresh leaves."""
    names = {"dsc": ("src_depth", "tgt_depth"), "rsc": ("tgt_depth",), "dc": ("tgt_depth", "small"), "smooth": ("tgt_depth",)}[term]
    return {n: (t[n] if dtype is None else t[n].to(dtype)).clone().requires_grad_(True) for n in names}


def _kernel(term, t, x):
    """-> (value [B], count [B] | None)"""
    if term == "dsc":
        return ops.depth_stereo_consistency(x["src_depth"], x["tgt_depth"], t["src_mask"], t["Kinv"], t["proj"], t["back"][:, 2], t["intr"])
    if term == "rsc":
        return ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], x["tgt_depth"], t["Kinv"], t["proj"])
    if term == "dc":
        return ops.depth_consistency(x["tgt_depth"], x["small"])
    return ops.edge_aware_smoothness(x["tgt_depth"], t["tgt_rgb"]), None


def _composition(term, t, x):
    """Today's loss_blocks function with per_item=True -> value [B]."""
    if term == "dsc":
        return lb.depth_stereo_consistency_loss(x["src_depth"].unsqueeze(1), x["tgt_depth"].unsqueeze(1), t["src_mask"], None, t["pose"],
                                                t["intr"], pose_src2target=t["back"], per_item=True)
    if term == "rsc":
        return lb.rgb_stereo_consistency_loss(t["src_rgb"], t["tgt_rgb"], x["tgt_depth"], t["pose"], t["intr"], per_item=True)
    if term == "dc":
        return lb.depth_consistency_loss(x["tgt_depth"], x["small"], per_item=True)
    d = x["tgt_depth"]
    return torch.stack([lb.edge_aware_smoothness_loss([d[i:i + 1].unsqueeze(1)], t["tgt_rgb"][i:i + 1], 1) for i in range(d.shape[0])])


def _composition_count(term, t):
    """The size of the mask the composition forms, from its own pieces."""
    with torch.no_grad():
        B, H, W = t["tgt_depth"].shape
        if term == "dsc":
            moved = iv.transform_dmap(t["src_depth"], t["back"], t["intr"]) * t["src_mask"]
            warped, valid = lb._warp(moved.unsqueeze(1), t["tgt_depth"], t["pose"], t["intr"], "nearest")
            mask = (valid & lb._lower_two_thirds(valid.shape, valid.device)).unsqueeze(1) & (warped > 0.)
        elif term == "rsc":
            _, valid = lb._warp(t["src_rgb"], t["tgt_depth"], t["pose"], t["intr"], "bilinear")
            mask = valid & lb._lower_two_thirds(valid.shape, valid.device)
        else:
            mask = lb._lower_two_thirds(t["small"].shape, t["small"].device)
        return mask.reshape(B, -1).sum(1).float()


def _restatement(term, t, x):
    if term == "dsc":
        return LT.dsc64(x["src_depth"], x["tgt_depth"], t["src_mask"], t["Kinv"], t["proj"], t["back"][:, 2], t["intr"])[0]
    if term == "rsc":
        return LT.rsc64(t["src_rgb"], t["tgt_rgb"], x["tgt_depth"], t["Kinv"], t["proj"])[0]
    if term == "dc":
        return LT.dc64(x["tgt_depth"], x["small"])[0]
    return LT.smooth64(x["tgt_depth"], t["tgt_rgb"])


def _weights(B, like):
    return torch.arange(1, B + 1, dtype=like.dtype, device=like.device)   # a different incoming gradient per item


def _run(fn, term, t, dtype=None):
    """-> (value [B] detached, {name: gradient}) of one side, the items weighted 1, 2, ..."""
    x = _leaves(term, t, dtype)
    value = fn(term, t, x)
    value = value[0] if isinstance(value, tuple) else value
    (value * _weights(value.shape[0], value)).sum().backward()
    return value.detach(), {n: v.grad for n, v in x.items()}


@functools.lru_cache(maxsize=None)
def _reference(term, shape):
    """The float64 restatement's value and gradients, once per (term, shape)."""
    cpu, _ = _inputs(shape)
    return _run(_restatement, term, cpu, torch.float64)


def _applies(term, shape):
    return term != "dc" or shape[1] >= 4


CASES = [(term, shape) for term in TERMS for shape in LT.SHAPES if _applies(term, shape)]


@pytest.mark.parametrize("term,shape", CASES)
def test_mask_count_is_the_compositions(dev, term, shape):
    """(The smoothness term has no mask: its denominators are the constants (H - 1) W and H (W - 1); nothing to count.)"""
    if term == "smooth":
        return
    _, t = _inputs(shape)
    _, count = _kernel(term, t, {n: t[n] for n in ("src_depth", "tgt_depth", "small")})
    want = _composition_count(term, t)
    print(term, shape, "count", count.tolist(), "composition", want.tolist())
    assert torch.equal(count, want) and not count.requires_grad
    assert bool((count > 0).all())


@pytest.mark.parametrize("term,shape", CASES)
def test_against_float64(dev, term, shape):
    _, t = _inputs(shape)
    v64, g64 = _reference(term, shape)
    vk, gk = _run(_kernel, term, t)
    vc, gc = _run(_composition, term, t)
    vk, vc = vk.double().cpu(), vc.double().cpu()
    assert bool(torch.isfinite(v64).all())
    err_k, e_ref = (vk - v64).abs(), (vc - v64).abs()
    ulp = torch.from_numpy(np.spacing(v64.abs().numpy().astype(np.float32)).astype(np.float64))
    print(term, shape, "value", vk.tolist(), "float64", v64.tolist(), "kernel error", err_k.tolist(), "E_ref", e_ref.tolist(),
          "ulp", ulp.tolist())
    worst = {}
    for n in g64:
        k, c, r = gk[n].double().cpu(), gc[n].double().cpu(), g64[n]
        assert k.shape == r.shape and bool(torch.isfinite(r).all())
        worst[n] = (float((k - r).abs().max()), float((c - r).abs().max()), float(r.abs().max()))
        print(term, shape, "gradient", n, "kernel max error %.3e  E_ref max %.3e  largest gradient %.3e" % worst[n])
    assert bool((err_k <= 2 * e_ref + 4 * ulp).all()), (term, shape, err_k.tolist(), e_ref.tolist())
    for n, (ek, er, big) in worst.items():
        assert ek <= 2 * er + 1e-6 * big, (term, shape, n, ek, er, big)


@pytest.mark.parametrize("term", TERMS)
def test_repeats(dev, term):
    """Two calls: the value and every gradient written without atomics carry the same bits; the scattered src_depth gradient of the
    depth-stereo term agrees to 1e-6 relative (of its largest element).  Under no_grad the same forward runs."""
    shape = (2, 64, 96)
    _, t = _inputs(shape)
    (v1, g1), (v2, g2) = _run(_kernel, term, t), _run(_kernel, term, t)
    assert torch.equal(v1, v2)
    for n in g1:
        if (term, n) == ("dsc", "src_depth"):
            assert float((g1[n] - g2[n]).abs().max()) <= 1e-6 * float(g1[n].abs().max())
        else:
            assert torch.equal(g1[n], g2[n]), (term, n)
    with torch.no_grad():
        plain = _kernel(term, t, {n: t[n] for n in ("src_depth", "tgt_depth", "small")})
    assert torch.equal(plain[0] if isinstance(plain, tuple) else plain, v1) and v1.dtype == torch.float32


def test_tie_goes_to_the_first_element(dev):
    g = torch.Generator().manual_seed(3)
    large = (10.0 + 20.0 * torch.rand(1, 8, 8, generator=g)).to(dev)
    large[0, 1, 2] = large[0, 2, 1] = large[0, 3, 3] = 5.0          # three equal minima in block (0, 0)
    large[0, 4:8, 4:8] = 7.0                                          # a block of sixteen equal depths
    small = torch.full((1, 2, 2), 9.0, device=dev)
    xk, xc = large.clone().requires_grad_(True), large.clone().requires_grad_(True)
    ops.depth_consistency(xk, small)[0].sum().backward()
    lb.depth_consistency_loss(xc, small, per_item=True).sum().backward()
    hit = xk.grad[0] != 0
    assert int(hit.sum()) == 4 and bool(hit[1, 2]) and bool(hit[4, 4]) and not bool(hit[2, 1]) and not bool(hit[3, 3])
    assert torch.equal(hit, xc.grad[0] != 0)
    assert torch.allclose(xk.grad, xc.grad, rtol=1e-5, atol=0)


def test_empty_mask_is_nan_for_its_item_alone(dev):
    shape = (2, 36, 48)
    _, t = _inputs(shape)
    x = {n: t[n] for n in ("src_depth", "tgt_depth", "small")}
    clean = {term: _kernel(term, t, x) for term in ("dsc", "rsc")}
    # depth-stereo: the source mask of item 1 is empty;  RGB: item 1 is so near that every pixel lands outside the source
    t_dsc = dict(t, src_mask=t["src_mask"].clone())
    t_dsc["src_mask"][1] = 0.0
    near = dict(x, tgt_depth=x["tgt_depth"].clone())
    near["tgt_depth"][1] = 0.01
    for term, tt, xx in (("dsc", t_dsc, x), ("rsc", t, near)):
        value, count = _kernel(term, tt, xx)
        want = _composition(term, tt, xx)
        print(term, "value", value.tolist(), "count", count.tolist(), "composition", want.tolist())
        assert float(count[1]) == 0.0 and bool(torch.isnan(value[1])) and bool(torch.isnan(want[1]))
        assert torch.equal(value[0], clean[term][0][0]) and torch.equal(count[0], clean[term][1][0])


@pytest.mark.parametrize("term", TERMS)
def test_non_finite_depths_stay_in_their_item(dev, term):
    shape = (2, 36, 48)
    _, t = _inputs(shape)
    x = {n: t[n] for n in ("src_depth", "tgt_depth", "small")}
    clean = _kernel(term, t, x)[0]
    cases = [("tgt_depth", ((0, 20, 10, float("nan")), (0, 30, 5, float("inf"))))]
    if term == "dsc":
        cases.append(("src_depth", ((0, 25, 20, float("nan")), (0, 28, 30, float("inf")))))
        cases.append(("tgt_depth", ((0, 2, 10, float("nan")),)))   # behind a zero mask (the top third): NaN * 0 is still NaN
    for name, pokes in cases:
        xx = dict(x, **{name: x[name].clone()})
        for b, i, j, v in pokes:
            xx[name][b, i, j] = v
        value = _kernel(term, t, xx)[0]
        want = _composition(term, t, xx)
        print(term, name, pokes, "value", value.tolist(), "composition", want.tolist())
        assert torch.equal(torch.isfinite(value), torch.isfinite(want)), (term, name)
        assert torch.equal(value[1], clean[1]) and bool(torch.isfinite(value[1]))


def test_two_rows_are_both_kept(dev):
    """H = 2: int(2 / 3) = 0, the top-third rule cuts no row."""
    _, t = _inputs((1, 2, 2))
    _, valid = lb._warp(t["src_rgb"], t["tgt_depth"], t["pose"], t["intr"], "bilinear")
    _, count = ops.rgb_stereo_consistency(t["src_rgb"], t["tgt_rgb"], t["tgt_depth"], t["Kinv"], t["proj"])
    assert float(count[0]) == float(valid.sum()) and bool(valid[0, 0].any()), valid


def test_remainder_rows_and_columns_get_no_gradient(dev):
    _, t = _inputs((3, 17, 23))
    x = _leaves("dc", t)
    assert tuple(x["small"].shape) == (3, 4, 5)
    ops.depth_consistency(x["tgt_depth"], x["small"])[0].sum().backward()
    g = x["tgt_depth"].grad
    assert float(g[:, 16:].abs().max()) == 0.0 and float(g[:, :, 20:].abs().max()) == 0.0
    assert int((g != 0).sum()) == int((x["small"].grad != 0).sum()) == 3 * 3 * 5   # (rows 1 .. 3 of the small map are kept)


def test_refusals_by_name(dev):
    _, t = _inputs((1, 4, 4))

    def leaf(n):
        return t[n].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="rgb_stereo_consistency: src_rgb requires grad"):
        ops.rgb_stereo_consistency(leaf("src_rgb"), t["tgt_rgb"], t["tgt_depth"], t["Kinv"], t["proj"])
    with pytest.raises(RuntimeError, match="rgb_stereo_consistency: tgt_rgb requires grad"):
        ops.rgb_stereo_consistency(t["src_rgb"], leaf("tgt_rgb"), t["tgt_depth"], t["Kinv"], t["proj"])
    for name in ("src_mask", "Kinv", "proj", "intr"):
        args = {n: (leaf(n) if n == name else t[n]) for n in ("src_depth", "tgt_depth", "src_mask", "Kinv", "proj", "intr")}
        with pytest.raises(RuntimeError, match=f"depth_stereo_consistency: {name} requires grad"):
            ops.depth_stereo_consistency(args["src_depth"], args["tgt_depth"], args["src_mask"], args["Kinv"], args["proj"],
                                         t["back"][:, 2], args["intr"])
    with pytest.raises(RuntimeError, match="depth_stereo_consistency: pose_row requires grad"):
        ops.depth_stereo_consistency(t["src_depth"], t["tgt_depth"], t["src_mask"], t["Kinv"], t["proj"],
                                     t["back"][:, 2].clone().requires_grad_(True), t["intr"])
    with pytest.raises(RuntimeError, match="edge_aware_smoothness: rgb requires grad"):
        ops.edge_aware_smoothness(t["tgt_depth"], leaf("tgt_rgb"))
    with pytest.raises(RuntimeError, match="loss_blocks.edge_aware_smoothness_loss"):
        ops.edge_aware_smoothness(t["tgt_depth"], t["tgt_rgb"][:, :, :2, :2])
    x = leaf("tgt_depth")   # once_differentiable: a second-order gradient raises, it is not a constant
    (g,) = torch.autograd.grad(ops.edge_aware_smoothness(x, t["tgt_rgb"]).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_a_map_beyond_the_size_limit_is_refused_for_its_size(dev):
    """Beyond H W = 2^24 the workspace query answers 0 and the binding passes no workspace at all: the entry refuses the size, which
    it judges before it looks at its workspace.  Nothing is launched and nothing of the (uninitialised) maps is read."""
    H, W = 4097, 4096
    for call in (lambda: _native.loss_smooth(torch.empty((1, H, W), device=dev), torch.empty((1, 3, H, W), device=dev)),
                 lambda: _native.flow_photo(torch.empty((1, 3, H, W), device=dev), torch.empty((1, 3, H, W), device=dev),
                                            torch.empty((1, 2, H, W), device=dev), torch.empty((1, 1, H, W), device=dev), 0.15, 0.85, 1.0)):
        with pytest.raises(RuntimeError) as refused:
            call()
        assert "2^24" in str(refused.value) and "workspace" not in str(refused.value)


# ---- BaseLoss ---------------------------------------------------------------------------------------------------------------------
def _base_run(dev, fused):
    inp = U.make_inputs()
    output, target = U.structure(inp, img_utils.gen_soft_label_torch, dev=dev)
    crit = BaseLoss(U.loss_cfg(), 0, fused_terms=fused)
    loss = crit(output, target)
    loss.backward()
    return loss.detach(), [v.grad for v in U.volumes(output)]


def _base64():
    """BaseLoss.forward restated in float64 on the CPU (the cross-entropy and the expectation as ops.dpv_soft_ce defines them, the
    four terms by util_loss_terms.py) -> (loss, gradients of the four volumes)."""
    inp = U.make_inputs()
    output, target = U.structure(inp, img_utils.gen_soft_label_torch, dtype=torch.float64)
    dc = torch.tensor(U.d_candi(), dtype=torch.float64).reshape(1, -1, 1, 1)
    mul, B = U.MULS, U.B

    def ce_and_depth(vol, labels, mask):
        ce = -(torch.stack(list(labels)) * vol).sum(1)
        m = mask[:, 0]
        cnt = (m == 1).sum((1, 2)).double()
        tot = torch.where(m != 0, ce * m, torch.zeros_like(ce)).sum((1, 2))
        return torch.where(cnt > 0, tot / cnt.clamp(min=1), torch.zeros_like(tot)).sum(), (dc * vol.exp()).sum(1)

    ce, small, large = 0, {}, {}
    for s, out, tg in (("l", output[0], target[0]), ("r", output[1], target[1])):
        lo, small[s] = ce_and_depth(out["output"][0], tg["soft_labels"], tg["masks"])
        hi, large[s] = ce_and_depth(out["output_refined"][0], tg["soft_labels_imgsize"], tg["masks_imgsizes"])
        ce = ce + lo + hi
    T = target[0]["T_left2right"].float()
    poses = {"l": T, "r": torch.inverse(T)}        # target to source, the target being the left / the right view
    other = {"l": "r", "r": "l"}
    side = {"l": target[0], "r": target[1]}
    dsc = rsc = dcl = smooth = 0
    for s in ("l", "r"):
        o = other[s]
        for dm, mk, ik in ((large, "masks_imgsizes", "intrinsics_up"), (small, "masks", "intrinsics")):
            K = side[s][ik].float()
            Kinv, proj, _ = LT.camera_matrices(K, poses[s], lb._inv3)
            dsc = dsc + LT.dsc64(dm[o], dm[s], side[o][mk][:, 0], Kinv, proj, poses[o][None, 2], K)[0].sum()
            if dm is large:
                rsc = rsc + LT.rsc64(side[o]["rgb"][:, -1], side[s]["rgb"][:, -1], large[s], Kinv, proj)[0].sum()
        dcl = dcl + LT.dc64(large[s], small[s])[0].sum()
        smooth = smooth + LT.smooth64(large[s], side[s]["rgb"][:, -1]).sum()
    loss = (ce / (2 * B)) * mul["ce_mul"] + (dsc * mul["dsc_mul"] + dcl * mul["dc_mul"] + rsc * mul["rsc_mul"] +
                                             smooth * mul["smooth_mul"]) / (2 * B)
    loss.backward()
    return loss.detach(), [v.grad for v in U.volumes(output)]


def test_base_loss_fused_against_the_reference(dev):
    """The criteria of test_loss_gpu.py::test_base_loss_against_the_reference, on the fused path."""
    g = golden("g24_loss.npz")
    loss, grads = _base_run(dev, fused=True)
    want = float(g["base_loss"])
    print("BaseLoss(fused_terms=True)", float(loss), "reference", want, "reference in float64", float(g["base_loss64"]))
    for name, v in zip(("left_lo", "left_hi", "right_lo", "right_hi"), grads):
        got, ref = v.double().cpu(), torch.from_numpy(g["base_grad_" + name]).double()
        per_pixel = (got - ref).pow(2).sum(1).flatten()
        allowed = int(per_pixel.numel() * 1e-3)   # pixels whose nearest tap or clamp flips: at most 0.1 % may be left out
        kept = per_pixel.sort().values[:per_pixel.numel() - allowed] if allowed else per_pixel
        rel_all, rel = float(per_pixel.sum().sqrt() / ref.norm()), float(kept.sum().sqrt() / ref.norm())
        print(name, "||g - g_ref|| / ||g_ref|| =", rel_all, "without the worst", allowed, "pixels:", rel)
        assert rel <= 1e-4, name
    assert abs(float(loss) - want) <= 1e-5 * abs(want)


def test_base_loss_fused_against_the_composition(dev):
    """Same device, same inputs: the loss within 1e-6 relative; every gradient element within 2 max E_ref + 1e-6 of the largest
    gradient, E_ref = the composition's own error against the float64 restatement of the whole loss; no pixel left out."""
    loss_f, grads_f = _base_run(dev, fused=True)
    loss_c, grads_c = _base_run(dev, fused=False)
    loss64, grads64 = _base64()
    print("BaseLoss fused", float(loss_f), "composition", float(loss_c), "float64", float(loss64))
    assert abs(float(loss_f) - float(loss_c)) <= 1e-6 * abs(float(loss_c))
    for name, f, c, r in zip(("left_lo", "left_hi", "right_lo", "right_hi"), grads_f, grads_c, grads64):
        f, c = f.double().cpu(), c.double().cpu()
        ek, er, big = float((f - r).abs().max()), float((c - r).abs().max()), float(r.abs().max())
        print(name, "fused max error %.3e  E_ref max %.3e  largest gradient %.3e  |fused - composition| max %.3e" %
              (ek, er, big, float((f - c).abs().max())))
        assert ek <= 2 * er + 1e-6 * big, name


def test_base_loss_fused_does_not_synchronise(dev):
    _base_run(dev, fused=True)   # (first call: the depth candidates are uploaded once and cached)
    torch.cuda.synchronize()
    output, target = U.structure(U.make_inputs(), img_utils.gen_soft_label_torch, dev=dev)
    crit = BaseLoss(U.loss_cfg(), 0, fused_terms=True)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(output, target)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert bool(torch.isfinite(loss)) and all(v.grad is not None for v in U.volumes(output))


def test_default_is_the_composition(dev, monkeypatch):
    calls = []
    for name in ("loss_dsc", "loss_rsc", "loss_dc", "loss_smooth"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    output, target = U.structure(U.make_inputs(), img_utils.gen_soft_label_torch, dev=dev)
    BaseLoss(U.loss_cfg(), 0)(output, target).backward()
    assert calls == []
    from pdepth_amd.losses import get_loss
    get_loss(U.loss_cfg(), 0)(output, target)
    assert calls == []
    BaseLoss(U.loss_cfg(), 0, fused_terms=True)(output, target)
    assert sorted(calls) == ["loss_dc"] * 2 + ["loss_dsc"] * 4 + ["loss_rsc"] * 2 + ["loss_smooth"] * 2
