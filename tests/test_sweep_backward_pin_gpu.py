"""GPU suite: the plane-sweep backward (csrc/sweep_bwd_body.hpp, run by sweep_bwd.hip and sweep_bwd_det.hip) held, element by
element, to float64 arithmetic at the kernel's own float32 sample positions, under the bound that tests/util_sweep_backward.py
derives from the kernel's roundings: g_ref and both g_src paths (float atomics, integer sum), both metrics, on the smallest
shapes at which each piece of the body can go wrong.  Beside it the project's max-norm rule, max|g - g64| <= 2 E_ref + eps32
max|g64|, with E_ref the error of torch's CPU float32 autograd of the same formula, measured here.  Everything asserted is printed."""
import functools
import importlib.util
import os

import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops, synth
import util_sweep_backward as U
from util_sweep_backward import EPS32, exact64_grads, oracle_grads, pin_check, to_dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("L2", "L1")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device(DEV)


# ---- the cases: name -> (batch dict, sigma) ------------------------------------------------------------------------------------
def _mk(config_id, B, V, C, D, H, W, pose="mono", mean=0.0, sigma=10.0, **kw):
    b = synth.make_batch(config_id, B, C=C, D=D, H=H, W=W, V=V, pose=pose, **kw)
    if mean:
        b["ref"], b["src"] = b["ref"] + mean, b["src"] + mean
    return b, sigma


def _extreme(kind):
    """The poses of tests/test_hip_parity.py::test_tiled_falls_back_to_gather_on_extreme_poses."""
    b = synth.make_batch(41, 2, C=12, D=16, H=40, W=72, V=2, pose="mono")
    t = b["t"].clone()
    if kind == "sideways":
        t[:, 0] = torch.tensor([6.0, 2.0, 0.0])
    else:
        t[:, 1] = torch.tensor([0.0, 0.0, -20.0])   # some planes end up behind the source camera
    b["t"] = t
    return b, 10.0


def _soak():
    spec = importlib.util.spec_from_file_location("soak_tool", os.path.join(REPO, "tools", "soak.py"))
    soak = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(soak)
    _, b = soak.replay_case(778, 98, spec=True, offset=True)   # tests/test_sweep_backward.py: the ill-conditioned soak input
    return b, 8.0


def _ordinary(i):
    from test_sweep_backward import CASES
    _, V, C, D, pose, cx_off = CASES[i]
    return _mk(23, 2, V, C, D, 24, 40, pose, cx_off=cx_off)


def _ordinary_name(i):
    from test_sweep_backward import CASES
    return "ordinary-" + "-".join(map(str, CASES[i][1:]))


_MAKERS = {
    "ragged_3x5": lambda: _mk(71, 1, 1, 1, 1, 3, 5),          # one ragged tile, dead lanes on the last pixel, seven padded channels
    "one_tile_16x16": lambda: _mk(72, 1, 1, 3, 8, 16, 16),
    "second_tile_17x33": lambda: _mk(73, 1, 1, 3, 8, 17, 33),  # one row / one column of a second tile
    "C9": lambda: _mk(74, 1, 2, 9, 16, 24, 40),               # 9 = 2 * 4 + 1: one live channel in the last pass (and 8 + 1 for g_ref's 8-wide pass)
    "C12": lambda: _mk(75, 1, 2, 12, 16, 24, 40),             # 12 = 3 * 4 = 8 + 4: full 4-wide passes, half an 8-wide one
    "D512": lambda: _mk(76, 1, 1, 3, 512, 17, 19),            # the ABI's plane cap, 96 KB of LDS
    "sigma_minus_3": lambda: _mk(77, 2, 2, 5, 8, 20, 24, sigma=-3.0),
    "mean_6_sigma": lambda: _mk(78, 1, 2, 6, 16, 24, 40, mean=6.0),   # S >> |e|: the A1 term
    "soak_778_98": _soak,
    "behind": lambda: _extreme("behind"),
    "sideways": lambda: _extreme("sideways"),
    "strided_leaf": lambda: _mk(32, 2, 2, 9, 8, 12, 20),      # ref = allv[:, -1], src = allv[:, :-1] of one leaf
}
for _i in range(8):
    _MAKERS[_ordinary_name(_i)] = functools.partial(_ordinary, _i)
for _n in ("A", "C", "E", "R"):
    _MAKERS[_n] = functools.partial(lambda n: (U.group_cases()[n], 10.0), _n)
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _MAKERS[name]()


@functools.lru_cache(maxsize=None)
def upstream(name, spike=False):
    """g_cost ~ N(0, 1), seed 5 (the upstream gradient of the older suites); spike: one value of 2^12 in item 0."""
    b, _ = case(name)
    B, V, C, H, W = b["src"].shape
    g = torch.randn(B, len(b["d_candi"]), H, W, generator=torch.Generator().manual_seed(5))
    if spike:
        g[0, len(b["d_candi"]) // 2, H // 2, W // 3] = 4096.0
    return g


@functools.lru_cache(maxsize=None)
def reference(name, metric, spike=False, dev=DEV):
    """The dict of exact64_grads (float64, on `dev`) of a case, with E_ref = (g_ref's, g_src's) max error of torch's CPU
    float32 autograd of oracle_cost against it, that evaluation checked against the bound on the way.  Read-only."""
    b, sigma = case(name)
    gup = upstream(name, spike)
    x = exact64_grads(b, gup, sigma, metric, dev=dev)
    r32, s32 = oracle_grads(b, gup, sigma, metric, torch.float32, "cpu")
    tag = "%s %s CPU float32 autograd" % (name, metric)
    pin_check(r32, x, "ref", tag + " g_ref")
    pin_check(s32, x, "src", tag + " g_src")
    x["E_ref"] = (U.max_err(r32, x, "ref"), U.max_err(s32, x, "src"))
    return x


def hip(dev, name, metric, deterministic, spike=False, src=None):
    """(g_ref, g_src) of ops.sweep_cost on a case; 'strided_leaf' goes through one leaf [B,V+1,C,H,W] as the model passes it."""
    b, sigma = case(name)
    d = to_dev(b, dev)
    gup = upstream(name, spike).to(dev)
    args = (d["K"], d["R"], d["t"], d["rays"], d["cxcy"], d["d_candi"], sigma)
    if name == "strided_leaf":
        allv = torch.cat([d["src"], d["ref"][:, None]], dim=1).requires_grad_(True)
        cost = ops.sweep_cost(allv[:, -1], allv[:, :-1], *args, feat_dist=metric, deterministic=deterministic)
        (cost * gup).sum().backward()
        return allv.grad[:, -1], allv.grad[:, :-1]
    ref = d["ref"].clone().requires_grad_(True)
    s = (d["src"] if src is None else src.to(dev)).clone().requires_grad_(True)
    cost = ops.sweep_cost(ref, s, *args, feat_dist=metric, deterministic=deterministic)
    (cost * gup).sum().backward()
    return ref.grad, s.grad


def _max_norm(tag, g, x, which):
    """-> '' or the complaint of the max-norm rule: max (|g - g64| - L1 allowance)+ <= 2 E_ref + eps32 max|g64|."""
    e, e_ref, big = U.max_err(g, x, which), x["E_ref"][which == "src"], float(x["g_" + which].abs().max())
    limit = 2 * e_ref + EPS32 * big
    print("%s: max error %.3e, E_ref %.3e, max |g64| %.3e, limit %.3e, max error / limit %.2f" % (tag, e, e_ref, big, limit, e / limit))
    return "" if e <= limit else "%s: max error %.3e > 2 E_ref + eps32 max|g64| = %.3e (E_ref %.3e)" % (tag, e, limit, e_ref)


def _allowance_cap(tag, x):
    share = U.allowance_share(x)
    print("%s: the L1 allowance touches %.4f %% of g_ref, %.4f %% of g_src" % (tag, 100 * share[0], 100 * share[1]))
    assert max(share) <= 1e-2, (tag, share)


@functools.lru_cache(maxsize=None)
def grads(name, metric, deterministic):
    """hip() of the plain case, once per path: read-only."""
    return hip(torch.device(DEV), name, metric, deterministic)


# ---- every element, every path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_every_element_within_the_bound(dev, name, metric):
    x = reference(name, metric)
    tag = "%s %s" % (name, metric)
    gr, gs = grads(name, metric, False)
    gr_d, gs_d = grads(name, metric, True)
    assert torch.equal(gr, gr_d)   # g_ref is the gather pass either way
    pin_check(gr, x, "ref", tag + " g_ref")
    pin_check(gs, x, "src", tag + " g_src atomic")
    pin_check(gs_d, x, "src", tag + " g_src deterministic", det=True)
    if metric == "L1":
        _allowance_cap(tag, x)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", NAMES)
def test_max_norm_rule(dev, name, metric):
    """max|g - g64| <= 2 E_ref + eps32 max|g64| for g_ref and both g_src paths, E_ref the same figure of torch's CPU float32
    autograd of oracle_cost, measured here (for L1 both are taken over the excess above the sign allowance).

    What this rule found.  With the box image and the g_ref sum in float32 the rule was missed on 12 of the 48 parameters, where
    a sum is long: g_ref by up to 1.09x (L2) and 1.91x (L1, D512), the float-atomic g_src by up to 2.63x (L2) and 4.22x (L1, D512;
    2.1x ... 2.7x at V = 4, C = 80, D = 128 and V = 2, D = 128), while the integer sum stayed at 0.38 or below.  No term was wrong -- every
    element was inside the per-element bound --, the order of the sums was: torch sums the D planes of a view with its cascade
    (the backward of expand() is a sum()) and E_ref is that cascade's error; g_ref added the V D terms of a pixel one after another
    in a float32 register and the atomics added a texel's contributions in float32 in their order of arrival (the same float32
    terms summed plane after plane on the host gave 1.90e-5 for D512 L2 and 9.282e-6 for ordinary-1-67-64-identity L2, the kernel's
    own figure to the digit, where torch.sum gives 3.6e-6 and 3.5e-6).  csrc/sweep_bwd_body.hpp now keeps both sums in double (the
    LDS box image of the float path, the g_ref register); on an MI355X max error / limit is at most 0.29 (g_ref) and 0.38 (both
    g_src paths) over the 48 parameters."""
    x = reference(name, metric)
    tag = "%s %s" % (name, metric)
    gr, gs = grads(name, metric, False)
    _, gs_d = grads(name, metric, True)
    missed = [m for m in (_max_norm(tag + " g_ref", gr, x, "ref"), _max_norm(tag + " g_src atomic", gs, x, "src"),
                          _max_norm(tag + " g_src deterministic", gs_d, x, "src")) if m]
    assert not missed, "\n".join(missed)


def _between_paths(tag, gs, gs_d, x):
    """The two paths' contributions are the same bits, only the sum differs: |det - atomic| <= eps32 n A0 + n N M_b 2^-59."""
    n, A0 = x["n_src"], x["A0_src"]
    bound = EPS32 * n * A0 + n * (x["N"] * 2.0 ** -59) * x["Mb"].reshape(-1, 1, 1, 1, 1)
    bound = torch.where(A0 > 0, bound, torch.zeros_like(bound))
    pin_check(gs_d, x, "src", tag + " deterministic against atomic", bound=bound, want=gs.double())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ("ragged_3x5", "C9", "D512", "mean_6_sigma", "ordinary-4-3-64-wide--5.0", "A", "R", "sideways"))
def test_the_two_g_src_paths_against_each_other(dev, name, metric):
    x = reference(name, metric)
    _, gs = grads(name, metric, False)
    _, gs_d = grads(name, metric, True)
    _between_paths("%s %s" % (name, metric), gs, gs_d, x)


@pytest.mark.parametrize("metric", METRICS)
def test_dynamic_range_inside_one_item(dev, metric):
    """One g_cost value of 2^12 in otherwise N(0, 1) input: the integer sum's exponent follows the item's maximum, its bound carries
    the quantisation term n N M_b 2^-59 with that maximum in M_b; the float atomics' bound is the plain one."""
    name = "R"
    x = reference(name, metric, spike=True)
    tag = "%s %s, one g_cost of 2^12" % (name, metric)
    gr, gs = hip(dev, name, metric, False, spike=True)
    _, gs_d = hip(dev, name, metric, True, spike=True)
    quant = float((x["n_src"].amax() * x["N"] * 2.0 ** -59) * x["Mb"].max())
    print("%s: M_b %s, N %d, largest quantisation term %.3e" % (tag, ["%.3e" % m for m in x["Mb"].tolist()], x["N"], quant))
    pin_check(gr, x, "ref", tag + " g_ref")
    pin_check(gs, x, "src", tag + " g_src atomic")
    pin_check(gs_d, x, "src", tag + " g_src deterministic", det=True)
    _between_paths(tag, gs, gs_d, x)
    if metric == "L1":
        _allowance_cap(tag, x)


# ---- the non-finite contract of the atomic path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_a_nan_texel_reaches_its_own_samples_only(dev, metric):
    """A NaN in src.  L1: the branches e > 0 / e < 0 both fail, the sample contributes 0 (torch's abs backward: sign(nan) == 0) and
    every gradient is finite -- the float64 reference does the same, so the bound applies as it is.  L2: NaN at exactly the texels
    and the pixels the NaN's samples reach, as torch's CPU autograd of oracle_cost has it on the same input; every other element
    within the bound of the clean input's reference."""
    name = "C9"
    b, sigma = case(name)
    src = b["src"].clone()
    src[0, 1, 8, 11, 17] = float("nan")   # the only live channel of the scatter's third pass
    gup = upstream(name)
    gr, gs = hip(dev, name, metric, False, src=src)
    r32, s32 = oracle_grads(dict(b, src=src), gup, sigma, metric, torch.float32, "cpu")
    nan_r, nan_s = torch.isnan(r32).to(dev), torch.isnan(s32).to(dev)
    print("%s %s: torch has %d NaN in g_ref, %d in g_src; the kernel %d, %d"
          % (name, metric, int(nan_r.sum()), int(nan_s.sum()), int(torch.isnan(gr).sum()), int(torch.isnan(gs).sum())))
    assert torch.equal(torch.isnan(gr), nan_r) and torch.equal(torch.isnan(gs), nan_s)
    if metric == "L1":
        assert not bool(nan_r.any()) and not bool(nan_s.any())
        x = exact64_grads(dict(b, src=src), gup, sigma, metric, dev=DEV)
    else:
        assert bool(nan_r.any()) and bool(nan_s.any())
        assert int(nan_r[:, :8].sum()) == 0 and int(nan_s[:, :, :8].sum()) == 0 and int(nan_s[:, 0].sum()) == 0   # its own channel and view
        x = reference(name, metric)
        gr, gs = torch.where(nan_r, x["g_ref"].float(), gr), torch.where(nan_s, x["g_src"].float(), gs)
    pin_check(gr, x, "ref", "%s %s, a NaN texel: g_ref" % (name, metric))
    pin_check(gs, x, "src", "%s %s, a NaN texel: g_src" % (name, metric))
