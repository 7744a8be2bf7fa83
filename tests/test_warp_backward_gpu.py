"""GPU suite: ops.warp_feature(differentiable=True) -- the backward of csrc/warp_bwd.hip, both paths (float atomics and the
order-independent integer sum) -- against the float64 autograd oracle of tests/util_warp_backward.py, on every texel, within
(4 + n) eps32 A (exactly 0 where no tap lands): the bound the reference's own float32 backward is shown to meet in
test_warp_backward_host.py.  Nothing is masked out: every position of the cases is finite."""
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops
import util_warps as U
import util_warp_backward as WB

pytestmark = pytest.mark.gpu

CASES = ("chunks_clamped_to_D", "chunks16_ragged_planes", "D128", "off_centre_items", "wide", "behind", "model_shape")
PATHS = [False, True]
PATH_IDS = ["atomic", "det"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _cam(b, dev, items=None):
    sel = (lambda x: x) if items is None else (lambda x: x[items])
    return [sel(b[k]).to(dev) for k in ("K", "R", "t", "rays", "cxcy")]


def _forward(b, dev, src, deterministic, items=None):
    return ops.warp_feature(src, *_cam(b, dev, items), b["d_candi"], differentiable=True, deterministic=deterministic)


def _grad(b, dev, g_out, deterministic, src=None, items=None):
    """-> (out, g_src) on the device: one forward under autograd, one backward."""
    leaf = (b["src"] if src is None else src)
    leaf = (leaf if items is None else leaf[items]).to(dev).requires_grad_(True)
    out = _forward(b, dev, leaf, deterministic, items)
    g, = torch.autograd.grad(out, leaf, (g_out if items is None else g_out[items]).to(dev))
    return out.detach(), g


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", CASES)
def test_gradient_against_float64(dev, name, deterministic):
    b, ref = U.warp_feature_case(name), WB.reference(name)
    out, g = _grad(b, dev, ref["g_out"], deterministic)
    assert g.dtype == torch.float32 and g.shape == b["src"].shape
    with torch.no_grad():
        plain = ops.warp_feature(b["src"].to(dev), *_cam(b, dev), b["d_candi"])
    assert torch.equal(out, plain), "the forward under autograd is the no-grad kernel, bit for bit"
    WB.check(g, ref, f"{name}, {'det' if deterministic else 'atomic'}")


@pytest.mark.parametrize("deterministic", PATHS, ids=PATH_IDS)
def test_expanded_view_sums_over_the_views(dev, deterministic):
    """src[:, :1].expand(-1, 2, ...) as a non-leaf of a leaf: the gradient comes back in the expanded shape and autograd sums it
    over the views (one more float32 rounding, of at most eps32 / 2 (A_0 + A_1): inside the sum of the two views' bounds, which
    are twice what the derivation needs)."""
    name = "strided_views"
    b, pos, g_out = U.warp_feature_case(name), WB.positions(name), WB.upstream(name)
    rep = b["src"][:, :1].expand(-1, 2, -1, -1, -1).contiguous()
    g64, A = WB.oracle_grads(b, pos, g_out, src=rep)
    bound = ((4 + WB.tap_counts(*pos)) * WB.EPS32 * A).sum(dim=1)
    leaf = b["src"].to(dev).requires_grad_(True)
    out = _forward(b, dev, leaf[:, :1].expand(-1, 2, -1, -1, -1), deterministic)
    out.backward(g_out.to(dev))
    assert bool((leaf.grad[:, 1] == 0).all())
    WB.check(leaf.grad[:, 0], None, f"expanded view, {'det' if deterministic else 'atomic'}", bound=bound, want=g64.sum(dim=1))


# ---- the two paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("behind", "model_shape"))
def test_deterministic_path_repeats_its_bits(dev, name):
    b, ref = U.warp_feature_case(name), WB.reference(name)
    _, g1 = _grad(b, dev, ref["g_out"], True)
    _, g2 = _grad(b, dev, ref["g_out"], True)
    assert torch.equal(g1, g2)


def test_deterministic_item_does_not_depend_on_the_batch(dev):
    name = "off_centre_items"
    b, ref = U.warp_feature_case(name), WB.reference(name)
    _, whole = _grad(b, dev, ref["g_out"], True)
    for i in range(b["src"].shape[0]):
        _, alone = _grad(b, dev, ref["g_out"], True, items=slice(i, i + 1))
        assert torch.equal(alone[0], whole[i]), i


@pytest.mark.parametrize("name", ("behind", "model_shape"))
def test_atomic_path_repeats_within_the_bound(dev, name):
    """Each call is within half the bound of float64 (the bound is twice the derivation): two calls differ by the bound at most."""
    b, ref = U.warp_feature_case(name), WB.reference(name)
    _, g1 = _grad(b, dev, ref["g_out"], False)
    _, g2 = _grad(b, dev, ref["g_out"], False)
    assert bool(((g1 - g2).abs().cpu().double() <= ref["bound"]).all())


# ---- a non-finite upstream gradient ------------------------------------------------------------------------------------------------
def _poisoned(name, item):
    """g_out with one NaN, at a sample of batch item `item` with all four taps inside -> (g_out, (b, v, k), its texels)."""
    b, (ix, iy), g = U.warp_feature_case(name), WB.positions(name), WB.upstream(name).clone()
    B, V, D, H, W = g.shape
    full = (U.tap_mask(ix, iy, H, W) == 15)[item]
    v, k, y, x = (int(i) for i in full.nonzero()[len(full.nonzero()) // 2])
    g[item, v, k, y, x] = float("nan")
    taps = [int(idx[0, 0]) for inside, idx in WB.tap_indices(ix[item, v, k, y, x].reshape(1, 1), iy[item, v, k, y, x].reshape(1, 1), H, W)]
    return g, (item, v, k), sorted(taps)


def test_atomic_path_keeps_a_nan_in_the_texels_it_reaches(dev):
    name = "off_centre_items"
    b = U.warp_feature_case(name)
    g_out, (i, v, k), taps = _poisoned(name, 1)
    _, g = _grad(b, dev, g_out, False)
    nan = torch.isnan(g).cpu()
    assert sorted(int(t) for t in nan[i, v, k].flatten().nonzero().flatten()) == taps and len(taps) == 4
    nan[i, v, k] = False
    assert not bool(nan.any()) and bool(torch.isfinite(g).cpu()[~torch.isnan(g).cpu()].all())


def test_deterministic_path_turns_the_item_into_nan_and_no_other(dev):
    name = "off_centre_items"
    b, ref = U.warp_feature_case(name), WB.reference(name)
    g_out, (i, _, _), _ = _poisoned(name, 1)
    _, clean = _grad(b, dev, ref["g_out"], True)
    _, g = _grad(b, dev, g_out, True)
    assert bool(torch.isnan(g[i]).all())
    for j in range(g.shape[0]):
        if j != i:
            assert torch.equal(g[j], clean[j]), j


def test_deterministic_zero_item_is_exactly_zero(dev):
    name = "off_centre_items"
    b, ref = U.warp_feature_case(name), WB.reference(name)
    g_out = ref["g_out"].clone()
    g_out[2] = 0
    _, clean = _grad(b, dev, ref["g_out"], True)
    _, g = _grad(b, dev, g_out, True)
    assert bool((g[2] == 0).all()) and torch.equal(g[:2], clean[:2])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    name = "chunks_clamped_to_D"
    b = U.warp_feature_case(name)
    src = b["src"].to(dev).requires_grad_(True)
    cam = dict(zip(("K", "R", "t", "rays", "cxcy"), _cam(b, dev)))
    with pytest.raises(RuntimeError, match="no backward"):   # the plain call stays refused
        ops.warp_feature(src, *cam.values(), b["d_candi"])
    for key in cam:
        c = dict(cam)
        c[key] = cam[key].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=f"{key} requires grad"):
            ops.warp_feature(src, *c.values(), b["d_candi"], differentiable=True)
    dc = ops.d_candi_tensor(b["d_candi"], dev).clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="d_candi requires grad"):
        ops.warp_feature(src, *cam.values(), dc, differentiable=True)
    # nothing requires grad, or grad mode is off: the plain path, no graph
    assert not ops.warp_feature(src.detach(), *cam.values(), b["d_candi"], differentiable=True).requires_grad
    with torch.no_grad():
        assert not ops.warp_feature(src, *cam.values(), b["d_candi"], differentiable=True).requires_grad
    # the backward is not differentiable a second time
    out = ops.warp_feature(src, *cam.values(), b["d_candi"], differentiable=True)
    g, = torch.autograd.grad(out.sum(), src, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---- what autograd hands the backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", PATHS, ids=PATH_IDS)
def test_non_contiguous_upstream_gradient(dev, deterministic):
    """.sum() over a permuted view of the output hands the backward a non-contiguous g_out: the same result as with its
    contiguous copy (within the bound for the atomics, bit for bit for the integer sum), and within the bound of float64."""
    name = "chunks16_ragged_planes"
    b, ref = U.warp_feature_case(name), WB.reference(name)
    w = ref["g_out"].to(dev).permute(0, 1, 2, 4, 3).contiguous()   # [B,V,D,W,H]
    leaf = b["src"].to(dev).requires_grad_(True)
    out = _forward(b, dev, leaf, deterministic)
    seen = []
    out.register_hook(lambda g: seen.append(g.is_contiguous()))
    (out.permute(0, 1, 2, 4, 3) * w).sum().backward()
    assert seen == [False]
    _, want = _grad(b, dev, ref["g_out"], deterministic)
    if deterministic:
        assert torch.equal(leaf.grad, want)
    else:
        assert bool(((leaf.grad - want).abs().cpu().double() <= ref["bound"]).all())
    WB.check(leaf.grad, ref, f"non-contiguous g_out, {'det' if deterministic else 'atomic'}")
