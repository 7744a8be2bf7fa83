"""GPU suite of the flow evaluation: ops.flow_metrics / ops.flow_resize (csrc/flow_metrics.hip) against the reference's own
evaluate_flow and a float64 statement of the formulas (fixture g30), the resized flow, reproducibility, the semantics on
hand-written maps, an unaligned truth, utils.flow_utils and harness.validate_flow without a host synchronisation.

Parity, per case, form and item.  The mask sums and the three bad-pixel counts (recovered as rate * sum(m) / 100, rounded) equal
the fixture exactly: the inputs are built so that no pixel is near a threshold (tests/util_flow_metrics.py).  Every mean and
rate: |hip - f64| <= max(|ref32 - f64|, bound), ref32 the reference's float32 run, with the derived
    bound = 8 * 2^-24 * (max |rescaled pred| + max |gt_uv|) + 4 * 2^-24 * |f64|
(the four-tap float interpolation and the subtraction lose at most a few ulp of the largest operand per pixel, a mean cannot be
further off than its worst pixel; U.bound computes it from the inputs).  flow_up per element: within 4 * 2^-24 *
max |rescaled pred| of the float64 resize."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pdepth_amd
from pdepth_amd import harness, ops, synth
from pdepth_amd.models.pwclite import PWCLite
from pdepth_amd.utils import flow_utils
from util import golden
import util_flow_metrics as U

pytestmark = pytest.mark.gpu
# OBSERVED (MI355X): worst err / bound over the 21 parity tests 0.012 (tiny, move; 0.005 or less in the cases of more than one
# workgroup): the bound allows every pixel its worst case with one sign, the errors of a mean largely cancel.  flow_up: worst
# err / (4 eps32 max |rescaled pred|) 0.811 (mixed), align_corners 0.736 (wide); the identity case 0.372, the rescale's rounding alone
NAN = float("nan")
MEANS = (0, 1, 2, 3, 4, 5)          # the columns of errors the reference returns (fixture: ref32 [B,6])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(dev):
    """name -> (numpy inputs, device inputs): built once, shared, never written."""
    out = {}
    for name in U.CASES:
        case = U.make_case(name)
        out[name] = (case, {k: torch.from_numpy(v).to(dev) for k, v in case.items()})
    return out


@pytest.fixture(scope="module")
def fixture():
    return golden("g30_flow_metrics.npz")


def _dev_form(d, form):
    return (d["gt"][:, :2].contiguous() if form == "uv" else d["gt"]), d["pred"], (d["move"] if form == "move" else None)


def _check(errors, counts, case, form, g, key, what):
    """errors [B,8], counts [B,5] (numpy) against the fixture's entries of `key` -> the worst err / bound."""
    errors, counts = np.float64(errors), np.float64(counts)
    f64, ref32, n, bad = g[key + "_f64"], np.float64(g[key + "_ref32"]), g[key + "_counts"], g[key + "_bad"]
    assert np.array_equal(np.isnan(counts), np.isnan(n)) and np.array_equal(counts[~np.isnan(n)], n[~np.isnan(n)]), (what, counts, n)
    assert np.array_equal(np.isnan(errors), np.isnan(f64)), (what, errors, f64)
    for j, (rate, m) in enumerate(((3, 0), (6, 3), (7, 4))):
        for b in range(U.B):
            if bad[b, j] >= 0:
                assert round(errors[b, rate] * counts[b, m] / 100.0) == bad[b, j], (what, b, rate, errors[b, rate], bad[b, j])
    worst = 0.0
    for b in range(U.B):
        gt, pred, _ = U.form_inputs(case, form, b)
        for j in range(8):
            if np.isnan(f64[b, j]):
                continue
            allowed = U.bound(gt, pred, f64[b, j])
            if j in MEANS and not np.isnan(ref32[b, j]):
                allowed = max(allowed, abs(ref32[b, j] - f64[b, j]))
            err = abs(errors[b, j] - f64[b, j])
            worst = max(worst, err / allowed)
            assert err <= allowed, (what, b, U.NAMES[j], errors[b, j], f64[b, j], err, allowed)
    return worst


@pytest.mark.parametrize("form", U.FORMS)
@pytest.mark.parametrize("name", list(U.CASES))
def test_parity(cases, fixture, name, form):
    case, d = cases[name]
    for k, v in U.checksums(name, case).items():
        assert fixture[k] == v, k
    gt, pred, move = _dev_form(d, form)
    errors, counts, flow_up = ops.flow_metrics(gt, pred, move_mask=move)
    assert errors.shape == (U.B, 8) and counts.shape == (U.B, 5) and flow_up is None
    worst = _check(errors.cpu().numpy(), counts.cpu().numpy(), case, form, fixture, f"{name}_{form}", f"{name} {form}")
    print(f"{name} {form}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(U.CASES))
def test_flow_up_resize_and_reproducibility(cases, name):
    case, d = cases[name]
    (h, w), (H, W) = U.CASES[name]
    gt, pred, move = _dev_form(d, "move")
    errors, counts, flow_up = ops.flow_metrics(gt, pred, move_mask=move, want_flow=True)
    M = np.abs(U.rescale64(case["pred"], (H, W))).max()
    err = np.abs(np.float64(flow_up.cpu().numpy()) - U.flow_up64(case["pred"], (H, W))).max()
    print(f"{name}: flow_up worst err / (4 eps32 max|rescaled pred|) = {err / (4 * U.EPS32 * M):.3f}")
    assert flow_up.shape == (U.B, 2, H, W) and err <= 4 * U.EPS32 * M
    if name == "same":   # the bits of pred / w * W in float32, by torch and by numpy (on the host: the device's division by a
        #                  Python number multiplies by its reciprocal)
        p = torch.from_numpy(case["pred"])
        assert torch.equal(flow_up.cpu(), torch.stack([p[:, 0] / w * W, p[:, 1] / h * H], dim=1))
        assert np.array_equal(flow_up.cpu().numpy()[:, 0], case["pred"][:, 0] / np.float32(w) * np.float32(W))
        assert np.array_equal(flow_up.cpu().numpy()[:, 1], case["pred"][:, 1] / np.float32(h) * np.float32(H))
    # with and without the map: the same bits
    e0, c0, none = ops.flow_metrics(gt, pred, move_mask=move)
    assert none is None and torch.equal(e0.view(torch.int32), errors.view(torch.int32)) and torch.equal(c0.view(torch.int32), counts.view(torch.int32))
    # flow_resize: the same sampling body
    assert torch.equal(ops.flow_resize(pred, (H, W)), flow_up)
    ac = ops.flow_resize(pred, (H, W), align_corners=True)
    want = F.interpolate(torch.from_numpy(U.rescale64(case["pred"], (H, W))), size=(H, W), mode="bilinear", align_corners=True).numpy()
    err = np.abs(np.float64(ac.cpu().numpy()) - want).max()
    print(f"{name}: align_corners worst err / (4 eps32 max|rescaled pred|) = {err / (4 * U.EPS32 * M):.3f}")
    assert err <= 4 * U.EPS32 * M
    assert torch.equal(flow_utils.resize_flow(pred, (H, W)), ac) and pred.data_ptr() != ac.data_ptr()
    # three calls: equal bits
    for _ in range(2):
        e2, c2, f2 = ops.flow_metrics(gt, pred, move_mask=move, want_flow=True)
        assert torch.equal(e2.view(torch.int32), errors.view(torch.int32)) and torch.equal(c2.view(torch.int32), counts.view(torch.int32))
        assert torch.equal(f2, flow_up)


def test_same_size_call_on_flow_up_reproduces_the_metrics(cases, dev):
    """ops.flow_metrics(gt, flow_up), the prediction now at the truth's size: the same bits as the call that made flow_up.  The
    same-size call rescales too -- (u / W) * W in float, the reference's two operations -- which returns u exactly where W and H
    are powers of two (both operations are exact) and may round where they are not (u / 3 * 3 != u for some u).  So the truth
    here is 16 x 32, the prediction 5 x 7 (the `tiny` case's) and 24 x 20: up and down, two workgroups per item."""
    H, W = 16, 32
    g = torch.Generator().manual_seed(41)
    for pred in (cases["tiny"][1]["pred"], (40.0 * torch.randn(U.B, 2, 24, 20, generator=g)).to(dev)):
        uv = 20.0 * torch.randn(U.B, 2, H, W, generator=g)
        valid = (torch.rand(U.B, 1, H, W, generator=g) < 0.6).float()
        noc = valid * (torch.rand(U.B, 1, H, W, generator=g) < 0.7).float()
        move = (torch.rand(U.B, H, W, generator=g) < 0.4).float().to(dev)
        gt = torch.cat([uv, valid, noc], dim=1).to(dev)
        errors, counts, flow_up = ops.flow_metrics(gt, pred, move_mask=move, want_flow=True)
        assert bool(torch.isfinite(errors).all())
        e1, c1, f1 = ops.flow_metrics(gt, flow_up, move_mask=move, want_flow=True)
        assert torch.equal(f1, flow_up)
        assert torch.equal(e1.view(torch.int32), errors.view(torch.int32)) and torch.equal(c1.view(torch.int32), counts.view(torch.int32))
        e2, c2, _ = ops.flow_metrics(gt[:, :2].contiguous(), flow_up)
        assert torch.equal(e2[:, 0], ops.flow_metrics(gt[:, :2].contiguous(), pred)[0][:, 0])


def test_an_item_does_not_depend_on_its_neighbour(cases):
    case, d = cases["odd_up"]
    gt, pred, move = _dev_form(d, "move")
    errors, counts, _ = ops.flow_metrics(gt, pred, move_mask=move)
    gt2, pred2 = gt.clone(), pred.clone()
    gt2[1, :2] += 5.0
    pred2[1] *= 0.5
    e2, c2, _ = ops.flow_metrics(gt2, pred2, move_mask=move)
    assert torch.equal(e2[0].view(torch.int32), errors[0].view(torch.int32)) and torch.equal(c2[0], counts[0])
    assert not torch.equal(e2[1], errors[1])
    e3, c3, _ = ops.flow_metrics(gt[:1], pred[:1], move_mask=move[:1])
    assert torch.equal(e3[0].view(torch.int32), errors[0].view(torch.int32)) and torch.equal(c3[0], counts[0])


def _hand(dev, gt, pred, move=None):
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=dev)   # noqa: E731
    e, c, _ = ops.flow_metrics(t(gt), t(pred), move_mask=t(move))
    return e.cpu().numpy(), c.cpu().numpy()


def test_semantics_on_hand_written_maps(dev):
    # 2 x 3 maps, the prediction at the truth's size; item 0: epe = (4, 4, 1, 0, 2, 5) against |gt| = (100, 20, ., ., ., 0).  The
    # errors sit in v, whose rescale v / 2 * 2 is exact (u / 3 * 3 need not be); the one u that is not 0 is 3: 3 / 3 * 3 = 3
    zeros = [[0.0] * 3, [0.0] * 3]
    gv0 = [[100.0, 20.0, 7.0], [3.0, -6.0, 0.0]]
    pv0 = [[104.0, 16.0, 8.0], [3.0, -4.0, 4.0]]
    pu0 = [[0.0, 0.0, 0.0], [0.0, 0.0, 3.0]]
    valid0 = [[1.0, 1.0, 1.0], [0.0, 1.0, 1.0]]
    noc0 = [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
    gv1 = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    pv1 = [[2.0, 2.0, 3.0], [4.0, 5.0, 8.0]]
    ones = [[1.0] * 3, [1.0] * 3]
    gt = [[zeros, gv0, valid0, noc0], [zeros, gv1, ones, ones]]
    pred = [[pu0, pv0], [zeros, pv1]]
    e, c = _hand(dev, gt, pred)
    # item 0: valid leaves out pixel (1, 0); epe over valid = (4 + 4 + 1 + 2 + 5) / 5; noc = (4 + 1 + 2) / 3; occ = (4 + 5) / 2
    assert c[0, :3].tolist() == [5.0, 3.0, 2.0] and np.isnan(c[:, 3:]).all()
    np.testing.assert_allclose(e[0, :3], [16.0 / 5, 7.0 / 3, 9.0 / 2], rtol=1e-6)
    # bad: epe 4 at |gt| 100 is not (4 %); epe 4 at |gt| 20 is (20 %); epe 5 at gt_uv == 0 is (the 1e-10 floor: no division by 0)
    assert e[0, 3] == np.float32(100.0 * 2 / 5)
    assert np.isnan(e[:, 4:]).all()                                  # no move mask: columns 4 to 7
    # item 1: noc == valid: epe_occ is 0 (0 / max(0, 1)), no pixel is bad
    assert c[1, :3].tolist() == [6.0, 6.0, 0.0] and e[1, 2] == 0.0 and e[1, 3] == 0.0
    np.testing.assert_allclose(e[1, :2], [0.5, 0.5], rtol=1e-6)
    # valid = 0 leaves a pixel out whatever its error: the same numbers with a wild prediction there
    pv0w = [[104.0, 16.0, 8.0], [1e6, -4.0, 4.0]]
    e2, c2 = _hand(dev, gt, [[pu0, pv0w], [zeros, pv1]])
    assert np.array_equal(e2, e, equal_nan=True) and np.array_equal(c2, c, equal_nan=True)
    # 2-channel truth: the plain mean over all six pixels, counts[0] = H W, everything else NaN
    e3, c3 = _hand(dev, [[zeros, gv0], [zeros, gv1]], pred)
    np.testing.assert_allclose(e3[:, 0], [16.0 / 6, 0.5], rtol=1e-6)
    assert np.isnan(e3[:, 1:]).all() and c3[:, 0].tolist() == [6.0, 6.0] and np.isnan(c3[:, 1:]).all()
    # an item with no valid pixel: NaN means and rate, count 0, epe_occ = 0 / max(0, 1) = 0 as in the reference; its neighbour untouched
    e4, c4 = _hand(dev, [[zeros, gv0, zeros, zeros], [zeros, gv1, ones, ones]], pred)
    assert np.isnan(e4[0, [0, 1, 3]]).all() and e4[0, 2] == 0.0 and c4[0, :3].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(e4[1], e[1], equal_nan=True) and np.array_equal(c4[1], c[1], equal_nan=True)
    # the move mask splits valid: move = column 0 and 1
    move = [[[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]], [[1.0] * 3, [1.0] * 3]]
    e5, c5 = _hand(dev, gt, pred, move)
    assert np.array_equal(e5[:, :4], e[:, :4]) and c5[0].tolist() == [5.0, 3.0, 2.0, 3.0, 2.0] and c5[1, 3:].tolist() == [6.0, 0.0]
    np.testing.assert_allclose(e5[0, 4:6], [(4.0 + 4 + 2) / 3, (1.0 + 5) / 2], rtol=1e-6)
    assert e5[0, 6] == np.float32(100.0 / 3) and e5[0, 7] == np.float32(50.0)
    assert e5[1, 6] == 0.0 and np.isnan(e5[1, [5, 7]]).all()          # nothing is static in item 1: 0 / 0


def test_unaligned_truth_takes_the_scalar_path(cases, dev):
    """A truth (and a move mask) whose storage starts one float past a 16-byte boundary: the same values, bit for bit."""
    case, d = cases["up4"]
    gt, pred, move = _dev_form(d, "move")
    assert gt.data_ptr() % 16 == 0 and (gt.shape[2] * gt.shape[3]) % 4 == 0
    errors, counts, _ = ops.flow_metrics(gt, pred, move_mask=move)
    flat = torch.empty(gt.numel() + 1, device=dev)
    gt1 = flat[1:].view_as(gt)
    gt1.copy_(gt)
    assert gt1.data_ptr() % 16 == 4 and gt1.is_contiguous()
    e1, c1, _ = ops.flow_metrics(gt1, pred, move_mask=move)
    assert torch.equal(e1.view(torch.int32), errors.view(torch.int32)) and torch.equal(c1, counts)
    flat_m = torch.empty(move.numel() + 1, device=dev)
    move1 = flat_m[1:].view_as(move)
    move1.copy_(move)
    e2, c2, _ = ops.flow_metrics(gt, pred, move_mask=move1)
    assert torch.equal(e2.view(torch.int32), errors.view(torch.int32)) and torch.equal(c2, counts)


@pytest.mark.parametrize("form", U.FORMS)
def test_evaluate_flow(cases, fixture, form):
    """utils.flow_utils.evaluate_flow on the reference's lists of HWC numpy maps and on device tensors: the batch means of the
    fixture, within the parity bound; items of two sizes in one list are evaluated per size group."""
    n = {"uv": 1, "masks": 4, "move": 6}[form]

    def want_and_bound(name):
        case, _ = cases[name]
        f64, ref32 = fixture[f"{name}_{form}_f64"], np.float64(fixture[f"{name}_{form}_ref32"])
        allowed = np.zeros((U.B, n))
        for b in range(U.B):
            gt, pred, _ = U.form_inputs(case, form, b)
            for j in range(n):
                allowed[b, j] = max(U.bound(gt, pred, f64[b, j]), abs(ref32[b, j] - f64[b, j]))
        return f64[:, :n], allowed

    for name in ("odd_up", "down"):
        case, d = cases[name]
        gt, pred, move = U.form_inputs(case, form)
        want, allowed = want_and_bound(name)
        lists = flow_utils.evaluate_flow([np.moveaxis(g, 0, -1) for g in gt], [np.moveaxis(p, 0, -1) for p in pred],
                                         None if move is None else list(move))
        dgt, dpred, dmove = _dev_form(d, form)
        tensors = flow_utils.evaluate_flow(dgt, dpred, dmove)
        for got in (lists, tensors):
            assert isinstance(got, list) and len(got) == n and all(isinstance(v, float) for v in got)
            assert (np.abs(np.asarray(got) - want.mean(0)) <= allowed.mean(0)).all(), (name, got, want.mean(0))
        assert lists == tensors
    # two sizes in one list
    (ca, _), (cb, _) = cases["odd_up"], cases["down"]
    ga, pa, ma = U.form_inputs(ca, form)
    gb, pb, mb = U.form_inputs(cb, form)
    hwc = lambda xs: [np.moveaxis(x, 0, -1) for x in xs]   # noqa: E731
    got = flow_utils.evaluate_flow(hwc(ga) + hwc(gb), hwc(pa) + hwc(pb), None if ma is None else list(ma) + list(mb))
    (wa, aa), (wb, ab) = want_and_bound("odd_up"), want_and_bound("down")
    want, allowed = np.concatenate([wa, wb]).mean(0), np.concatenate([aa, ab]).mean(0)
    assert len(got) == n and (np.abs(np.asarray(got) - want) <= allowed).all(), (got, want)


def test_validate_flow_runs_without_synchronising(dev):
    import types
    B, H, W, Hg, Wg = 2, 64, 128, 50, 140
    model = PWCLite(types.SimpleNamespace(upsample=True, n_frames=2, reduce_dense=True))
    synth.seed_weights(model, seed=29, gain=0.25)
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(31)
    batches = []
    for _ in range(2):
        img = torch.rand(B, 6, H, W, generator=g)
        uv = 6.0 * torch.randn(B, 2, Hg, Wg, generator=g)
        valid = (torch.rand(B, 1, Hg, Wg, generator=g) < 0.7).float()
        noc = valid * (torch.rand(B, 1, Hg, Wg, generator=g) < 0.8).float()
        move = (torch.rand(B, Hg, Wg, generator=g) < 0.3).float()
        batches.append((img.to(dev), torch.cat([uv, valid, noc], dim=1).to(dev), move.to(dev)))
    class Watched(torch.nn.Module):
        """the model, noting the sync-debug mode its forward runs under"""
        def __init__(self, inner):
            super().__init__()
            self.inner, self.modes = inner, []

        def forward(self, x):
            self.modes.append(torch.cuda.get_sync_debug_mode())
            return self.inner(x)

    watched = Watched(model)
    assert torch.cuda.get_sync_debug_mode() == 0
    res = harness.validate_flow(watched, batches)                     # (sets sync-debug "error" itself)
    assert torch.cuda.get_sync_debug_mode() == 0 and watched.modes == [2, 2]
    assert res["names"] == ops.FLOW_METRIC_NAMES and tuple(res["errors"]) == ops.FLOW_METRIC_NAMES and len(res["steps"]) == 2
    rows = []
    for (img, gt, move), step in zip(batches, res["steps"]):
        assert step["flow"].shape == (B, 2, H, W)
        e, c, _ = ops.flow_metrics(gt, step["flow"], move_mask=move)
        assert torch.equal(e, step["errors"]) and torch.equal(c, step["counts"])
        rows.append(e)
    table = torch.cat(rows).double().cpu().numpy()
    assert np.isfinite(table).all()
    for j, name in enumerate(ops.FLOW_METRIC_NAMES):
        assert res["errors"][name] == float(table[:, j].mean()), name
    # a 4-channel truth without a move mask, and a 2-channel truth: the columns they define
    r4 = harness.validate_flow(model, [(b[0], b[1]) for b in batches])
    t4 = torch.cat([s["errors"] for s in r4["steps"]]).double().cpu().numpy()
    assert r4["names"] == ops.FLOW_METRIC_NAMES[:4] and [r4["errors"][k] for k in r4["names"]] == [float(t4[:, j].mean()) for j in range(4)]
    assert np.isnan(t4[:, 4:]).all()
    r2 = harness.validate_flow(model, [(b[0], b[1][:, :2].contiguous()) for b in batches])
    assert r2["names"] == ("epe",) and np.isfinite(r2["errors"]["epe"])
    # the mode is restored when the loop raises
    with pytest.raises(RuntimeError, match="move mask"):
        harness.validate_flow(model, [(b[0], b[1][:, :2].contiguous(), b[2]) for b in batches])
    assert torch.cuda.get_sync_debug_mode() == 0
