"""GPU suite: the backward passes of the plane sweep and of the DPV reductions (csrc/sweep_bwd.hip, csrc/dpv_bwd.hip) behind
the autograd Functions of ops, against autograd of the oracle's formula (float64 and fp32), torch autograd of log_softmax /
exp / expectation, fixture g23 and a torch twin of BaseModel."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pdepth_amd
from pdepth_amd import _native, ops, synth
from oracle import ref_cpu as O
from util import golden
from util_sweep_backward import hip_grads, l1_allowance, oracle_grads, rel_err, to_dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


CASES = [  # metric, V, C, D, pose, cx_off
    ("L2", 1, 3, 16, "mono", 0.0),
    ("L2", 2, 67, 64, "stereo", 0.0),
    ("L1", 4, 80, 128, "wide", 0.0),
    ("L1", 1, 67, 64, "identity", 0.0),
    ("L2", 2, 80, 16, "mono", 7.5),
    ("L1", 2, 3, 128, "stereo", 0.0),
    ("L2", 4, 3, 64, "wide", -5.0),
    ("L2", 1, 67, 128, "identity", 0.0),
]


@pytest.mark.parametrize("metric,V,C,D,pose,cx_off", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_gradients_against_float64_oracle(dev, metric, V, C, D, pose, cx_off):
    b = synth.make_batch(23, 2, C=C, D=D, H=24, W=40, V=V, pose=pose, cx_off=cx_off)
    sigma = 10.0
    gup = torch.randn(2, D, 24, 40, generator=torch.Generator().manual_seed(5)).to(dev)
    r64, s64 = oracle_grads(b, gup, sigma, metric, torch.float64, dev)
    r32, s32 = oracle_grads(b, gup, sigma, metric, torch.float32, dev)
    ar, as_ = l1_allowance(b, gup, sigma, dev) if metric == "L1" else (None, None)
    # the bound is one fp32 can meet: autograd of the oracle in fp32 meets it
    assert rel_err(r32, r64, ar) <= 1e-4 and rel_err(s32, s64, as_) <= 1e-4, (rel_err(r32, r64, ar), rel_err(s32, s64, as_))
    gr, gs, _ = hip_grads(to_dev(b, dev), gup, sigma, metric)
    assert rel_err(gr, r64, ar) <= 1e-4, rel_err(gr, r64, ar)
    assert rel_err(gs, s64, as_) <= 1e-4, rel_err(gs, s64, as_)
    if metric == "L1":   # the allowance is the exception, not the rule: under 1 % of the elements (0.5 % at V = 4, D = 128)
        assert int((ar > 0).sum()) <= 1e-2 * ar.numel() and int((as_ > 0).sum()) <= 1e-2 * as_.numel()


def test_gradients_on_an_ill_conditioned_soak_input(dev):
    spec = importlib.util.spec_from_file_location("soak_tool", os.path.join(REPO, "tools", "soak.py"))
    soak = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(soak)
    shape, b = soak.replay_case(778, 98, spec=True, offset=True)   # (tests/test_soak_regressions.py: routed by the forward)
    sigma = 8.0
    B, D, H, W = shape["B"], len(b["d_candi"]), shape["H"], shape["W"]
    gup = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(6)).to(dev)
    r64, s64 = oracle_grads(b, gup, sigma, "L2", torch.float64, dev)
    gr, gs, _ = hip_grads(to_dev(b, dev), gup, sigma, "L2")
    assert rel_err(gr, r64) <= 1e-4 and rel_err(gs, s64) <= 1e-4, (rel_err(gr, r64), rel_err(gs, s64))


def test_gradients_match_fixture_g23(dev):
    g = golden("g23_sweep_backward.npz")
    cam = {k: torch.from_numpy(g[k]).to(dev) for k in ("K", "R", "t", "rays", "cxcy")}
    for metric in ("L2", "L1"):
        ref = torch.from_numpy(g["ref"]).to(dev).requires_grad_(True)
        src = torch.from_numpy(g["src"]).to(dev).requires_grad_(True)
        cost = ops.sweep_cost(ref, src, cam["K"], cam["R"], cam["t"], cam["rays"], cam["cxcy"], g["d_candi"], float(g["sigma"]),
                              feat_dist=metric, algo="direct")
        np.testing.assert_allclose(cost.detach().cpu().numpy(), g[metric + "_cost"], rtol=1e-4, atol=1e-3)
        (cost * torch.from_numpy(g[metric + "_gcost"]).to(dev)).sum().backward()
        for got, key in ((ref.grad, "_gref"), (src.grad, "_gsrc")):
            want = g[metric + key]
            assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), metric + key
    for bv_log in (True, False):
        tag = "lsm" if bv_log else "plain"
        x = torch.from_numpy(g[tag + "_in"]).to(dev).requires_grad_(True)
        y = ops.dpv_reduce(x, g["d_candi"], want_logp=True, want_depth=False)[0] if bv_log else x
        depth = ops.dpv_expect(y, g["d_candi"], BV_log=bv_log)
        (depth * torch.from_numpy(g[tag + "_gdepth"]).to(dev)).sum().backward()
        want = g[tag + "_grad"]
        np.testing.assert_allclose(x.grad.cpu().numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


@pytest.mark.parametrize("wants", [(True, False, False), (False, True, False), (False, False, True), (True, True, True),
                                   (False, True, True), (True, False, True)])
def test_sweep_dpv_gradients_in_any_combination(dev, wants):
    want_cost, want_logp, want_depth = wants
    d = to_dev(synth.make_batch(24, 2, C=67, D=64, H=32, W=48, V=2, pose="mono"), dev)
    gen = torch.Generator().manual_seed(7)
    gc, gl, gd = (torch.randn(2, 64, 32, 48, generator=gen).to(dev), torch.randn(2, 64, 32, 48, generator=gen).to(dev),
                  torch.randn(2, 32, 48, generator=gen).to(dev))

    def loss(outs):
        cost, logp, depth = outs
        tot = 0
        if want_cost:
            tot = tot + (cost * gc).sum()
        if want_logp:
            tot = tot + (logp * gl).sum()
        if want_depth:
            tot = tot + (depth * gd).sum()
        return tot

    args = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    ref, src = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
    loss(ops.sweep_dpv(ref, src, *args, want_cost=want_cost, want_logp=want_logp, want_depth=want_depth)).backward()
    # the same chain with the DPV tail in torch (the sweep backward is checked against the oracle above)
    ref2, src2 = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
    cost = ops.sweep_cost(ref2, src2, *args)
    logp = F.log_softmax(cost, dim=1)
    depth = (torch.exp(logp) * ops.d_candi_tensor(d["d_candi"], dev).view(1, -1, 1, 1)).sum(1)
    loss((cost, logp, depth)).backward()
    for a, b_ in ((ref.grad, ref2.grad), (src.grad, src2.grad)):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-5 * float(b_.abs().max()))


def _torch_reduce(x, dc):
    logp = F.log_softmax(x, dim=1)
    prob = torch.exp(logp)
    return logp, prob, (prob * dc.view(1, -1, 1, 1)).sum(1)


@pytest.mark.parametrize("addend", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
def test_dpv_reduce_gradients_against_torch(dev, addend, inplace):
    gen = torch.Generator().manual_seed(8)
    B, D, H, W = 2, 64, 16, 24
    x0 = (3 * torch.randn(B, D, H, W, generator=gen)).to(dev)
    a0 = torch.randn(B, D, H, W, generator=gen).to(dev)
    gl, gp, gd = (torch.randn(B, D, H, W, generator=gen).to(dev), torch.randn(B, D, H, W, generator=gen).to(dev),
                  torch.randn(B, H, W, generator=gen).to(dev))
    dc = torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0).astype(np.float32)).to(dev)
    x, a = x0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
    r = ops.dpv_reduce_ex(x, dc, addend=a if addend else None, want_logp=True, want_prob=True, want_depth=True, want_var=True,
                          want_quarter=True, inplace=inplace)
    assert not r["var"].requires_grad and not r["quarter"].requires_grad
    ((r["logp"] * gl).sum() + (r["prob"] * gp).sum() + (r["depth"] * gd).sum()).backward()
    xt, at = x0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
    lt, pt, dt = _torch_reduce(xt + at if addend else xt, dc)
    ((lt * gl).sum() + (pt * gp).sum() + (dt * gd).sum()).backward()
    torch.testing.assert_close(x.grad, xt.grad, rtol=1e-5, atol=1e-5 * float(xt.grad.abs().max()))
    if addend:
        torch.testing.assert_close(a.grad, at.grad, rtol=1e-5, atol=1e-5 * float(at.grad.abs().max()))
    torch.testing.assert_close(x0, x.detach())   # inplace is not honoured under autograd: the input is untouched
    # dpv_reduce (logp and depth)
    x = x0.clone().requires_grad_(True)
    logp, depth = ops.dpv_reduce(x, dc, want_logp=True, want_depth=True, inplace=inplace)
    ((logp * gl).sum() + (depth * gd).sum()).backward()
    xt = x0.clone().requires_grad_(True)
    lt, _, dt = _torch_reduce(xt, dc)
    ((lt * gl).sum() + (dt * gd).sum()).backward()
    torch.testing.assert_close(x.grad, xt.grad, rtol=1e-5, atol=1e-5 * float(xt.grad.abs().max()))


@pytest.mark.parametrize("bv_log", [True, False])
def test_dpv_expect_gradient_against_torch(dev, bv_log):
    gen = torch.Generator().manual_seed(9)
    B, D, H, W = 2, 32, 16, 24
    x0 = torch.randn(B, D, H, W, generator=gen).to(dev)
    gd = torch.randn(B, H, W, generator=gen).to(dev)
    dc = torch.from_numpy(synth.powerf(5.0, 40.0, D, 1.0).astype(np.float32)).to(dev)
    x = x0.clone().requires_grad_(True)
    (ops.dpv_expect(x, dc, BV_log=bv_log) * gd).sum().backward()
    xt = x0.clone().requires_grad_(True)
    ((torch.exp(xt) if bv_log else xt) * dc.view(1, -1, 1, 1)).sum(1).mul(gd).sum().backward()
    torch.testing.assert_close(x.grad, xt.grad, rtol=1e-5, atol=1e-6 * float(xt.grad.abs().max()))


@pytest.mark.parametrize("shape", [dict(B=2, C=67, D=64, H=32, W=48, V=2), dict(B=4, C=67, D=64, H=256, W=512, V=1)],
                         ids=["small", "headline"])
def test_forward_under_autograd_is_bit_identical(dev, shape):
    d = to_dev(synth.make_batch(25, shape["B"], C=shape["C"], D=shape["D"], H=shape["H"], W=shape["W"], V=shape["V"]), dev)
    args = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    ref, src = d["ref"].clone().requires_grad_(True), d["src"].clone().requires_grad_(True)
    with torch.no_grad():
        want = ops.sweep_dpv(d["ref"], d["src"], *args, want_cost=True, want_logp=True, want_depth=True, algo="auto")
        want_d = ops.sweep_dpv(d["ref"], d["src"], *args, want_cost=False, want_logp=False, want_depth=True, algo="auto")[2]
        want_c = ops.sweep_cost(d["ref"], d["src"], *args, algo="auto")
    got = ops.sweep_dpv(ref, src, *args, want_cost=True, want_logp=True, want_depth=True, algo="auto")
    for a, b_ in zip(got, want):
        assert a.requires_grad and torch.equal(a.detach(), b_)
    assert torch.equal(ops.sweep_dpv(ref, src, *args, want_cost=False, want_logp=False, want_depth=True, algo="auto")[2].detach(), want_d)
    assert torch.equal(ops.sweep_cost(ref, src, *args, algo="auto").detach(), want_c)
    x0 = want_c.clone()
    with torch.no_grad():
        w1 = ops.dpv_reduce(x0.clone(), d["d_candi"], want_logp=True, want_depth=True)
        w2 = ops.dpv_reduce(x0.clone(), d["d_candi"], want_logp=False, want_depth=True)
        w3 = ops.dpv_reduce_ex(x0.clone(), d["d_candi"], addend=x0 * 0.5, want_logp=True, want_prob=True, want_depth=True,
                               want_var=True, want_quarter=True)
        w4 = ops.dpv_expect(w1[0], d["d_candi"], BV_log=True)
    x = x0.clone().requires_grad_(True)
    g1 = ops.dpv_reduce(x, d["d_candi"], want_logp=True, want_depth=True)
    g2 = ops.dpv_reduce(x, d["d_candi"], want_logp=False, want_depth=True)
    g3 = ops.dpv_reduce_ex(x, d["d_candi"], addend=x0 * 0.5, want_logp=True, want_prob=True, want_depth=True, want_var=True,
                           want_quarter=True)
    g4 = ops.dpv_expect(w1[0].clone().requires_grad_(True), d["d_candi"], BV_log=True)
    assert torch.equal(g1[0].detach(), w1[0]) and torch.equal(g1[1].detach(), w1[1]) and g2[0] is None
    assert torch.equal(g2[1].detach(), w2[1])
    assert sorted(g3) == sorted(w3) and all(torch.equal(g3[k].detach(), w3[k]) for k in w3)
    assert torch.equal(g4.detach(), w4)


def test_gradients_reproducible(dev):
    d = to_dev(synth.make_batch(26, 2, C=67, D=64, H=64, W=96, V=2, pose="stereo"), dev)
    gup = torch.randn(2, 64, 64, 96, generator=torch.Generator().manual_seed(3)).to(dev)
    r1, s1, _ = hip_grads(d, gup, 10.0, "L2")
    r2, s2, _ = hip_grads(d, gup, 10.0, "L2")
    assert torch.equal(r1, r2)
    assert float((s1 - s2).abs().max()) <= 1e-6 * float(s1.abs().max())


def test_refusals(dev):
    d = to_dev(synth.make_batch(27, 1, C=8, D=16, H=16, W=32, V=1), dev)
    ref = d["ref"].clone().requires_grad_(True)
    for name in ("K", "R", "t", "rays", "cxcy"):
        dd = dict(d)
        dd[name] = d[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=name):
            ops.sweep_cost(ref, d["src"], dd["K"], dd["R"], dd["t"], dd["rays"], dd["cxcy"], d["d_candi"], 10.0)
    dc = torch.from_numpy(np.asarray(d["d_candi"], dtype=np.float32)).to(dev).requires_grad_(True)
    with pytest.raises(RuntimeError, match="d_candi"):
        ops.sweep_dpv(ref, d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc, 10.0)
    with pytest.raises(RuntimeError, match="d_candi"):
        ops.dpv_expect(torch.zeros(1, 16, 4, 4, device=dev, requires_grad=True), dc)
    packed = ops.pack_source(d["src"], n_planes=16)
    with pytest.raises(RuntimeError, match="NCHW"):
        ops.sweep_dpv(ref, packed, d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], 10.0)
    # still out of scope: no backward
    with pytest.raises(RuntimeError, match="no backward"):
        ops.warp_feature(torch.zeros(1, 1, 16, 16, 32, device=dev, requires_grad=True), d["K"], d["R"], d["t"], d["rays"], d["cxcy"],
                         d["d_candi"])


# ---- BaseModel trains ------------------------------------------------------------------------------------------------
def _torch_sweep_cost(ref, src, K, R, t, rays, cxcy, d_candi, sigma, feat_dist="L2", algo="auto", blas=None):
    B, V, C, H, W = src.shape
    dc = ops.d_candi_tensor(d_candi, ref.device)
    D = dc.numel()
    out = []
    for i in range(B):
        cost = 0
        for v in range(V):
            grid = O.plane_coords(K[i], R[i, v], t[i, v], rays[i], dc, cxcy[i, 0], cxcy[i, 1]).reshape(D, H, W, 2)
            warped = F.grid_sample(src[i, v].unsqueeze(0).expand(D, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                                   align_corners=False)
            cost = cost + ((warped - ref[i].unsqueeze(0)) ** 2).sum(1) / sigma
        out.append(cost)
    return torch.stack(out)


def _torch_dpv_reduce_ex(logits, d_candi=None, addend=None, want_logp=True, want_prob=False, want_depth=False, want_var=False,
                         want_quarter=False, inplace=False):
    x = logits if addend is None else logits + addend
    logp = F.log_softmax(x, dim=1)
    out = {"logp": logp}
    if want_prob:
        out["prob"] = torch.exp(logp)
    if want_depth:
        out["depth"] = (torch.exp(logp) * ops.d_candi_tensor(d_candi, x.device).view(1, -1, 1, 1)).sum(1)
    if want_quarter:
        out["quarter"] = F.interpolate(logp.detach(), scale_factor=0.25, mode="nearest")
    return out


def _torch_dpv_reduce(logits, d_candi, want_logp=True, want_depth=True, inplace=False):
    r = _torch_dpv_reduce_ex(logits, d_candi, want_depth=want_depth)
    return r["logp"], r.get("depth")


def _torch_dpv_expect(dpv, d_candi, BV_log=False):
    z = torch.exp(dpv) if BV_log else dpv
    return (z * ops.d_candi_tensor(d_candi, dpv.device).view(1, -1, 1, 1)).sum(1)


def _model_loss(model, inp, target):
    out = model([inp])[0]
    d = inp["d_candi"]
    loss = 0
    for bv in out["output"] + out["output_refined"]:
        depth = ops.dpv_expect(bv, d, BV_log=True)
        tgt = F.interpolate(target.unsqueeze(1), size=depth.shape[-2:], mode="nearest").squeeze(1)
        loss = loss + (depth - tgt).abs().mean()
    return loss


def test_base_model_trains(dev, monkeypatch):
    from pdepth_amd.models.get_model import get_model
    cfg = synth.default_cfg("default")
    torch.manual_seed(0)
    model = get_model(cfg, 0)
    synth.seed_weights(model, seed=31)
    model = model.to(dev).train()
    inp = to_dev(synth.make_model_input(3100, B=2, V=1, H=256, W=384, D=64, pose="mono"), dev)
    target = torch.rand(2, 256, 384, generator=torch.Generator().manual_seed(2)).to(dev) * 30 + 5
    twin = copy.deepcopy(model)
    loss = _model_loss(model, inp, target)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert grads and all(torch.isfinite(g).all() for g in grads.values())
    with monkeypatch.context() as mp:
        mp.setattr(ops, "sweep_cost", _torch_sweep_cost)
        mp.setattr(ops, "dpv_reduce_ex", _torch_dpv_reduce_ex)
        mp.setattr(ops, "dpv_reduce", _torch_dpv_reduce)
        mp.setattr(ops, "dpv_expect", _torch_dpv_expect)
        tloss = _model_loss(twin, inp, target)
        tloss.backward()
    assert abs(float(loss) - float(tloss)) <= 1e-3 * abs(float(tloss))
    checked = 0
    for n, p in twin.named_parameters():
        if not (n.startswith("base_encoder") or n.startswith("conv0") or n.startswith("base_decoder")) or p.grad is None:
            continue
        g, gt = grads[n], p.grad
        den = float(gt.norm())
        if den == 0:
            continue
        assert float((g - gt).norm()) <= 1e-3 * den, n
        checked += 1
    assert checked > 10
    # a few SGD steps on a fixed batch lower the loss
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    first = None
    for _ in range(4):
        opt.zero_grad()
        l = _model_loss(model, inp, target)
        first = float(l) if first is None else first
        l.backward()
        opt.step()
    assert float(_model_loss(model, inp, target)) < first
