"""GPU suite of the evaluation metrics: ops.depth_metrics (csrc/metrics.hip) in both forms against a float64 evaluation of the
formulas (fixture g25), the depth map of the volume form, the semantics of mask / zero / NaN / clamp / zero truth / empty item /
argument order, reproducibility, img_utils.depth_error, and harness.validate without a host synchronisation.

Tolerance of the parity test, per value: |hip - f64| <= max(|seq32 - f64|, 2e-6 |f64|) -- the device's fixed-order sums may not
be worse than the reference's sequential float sums on the same data (seq32: fixture source (b)); the floor is about 30 times
the 2^-24 rounding of a value.  The generator asserts what this rests on (the scale-invariant error's difference keeps at
least 5 % of its first term, at least 25 % of the pixels are valid).  The volume form forms its prediction on the device
(float32 sums of 16 products, a few ulp from the fixture's correctly rounded expectation): an error of ~1e-7 relative per
pixel with no common sign, far below the floor after the mean over >= 43 pixels.
Observed on an MI355X (max over cases, items and the nine values of |hip - f64| / |f64|): see OBSERVED below."""
import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import harness, ops, synth
from pdepth_amd.models.get_model import get_model
from pdepth_amd.utils import img_utils
from util import golden
import util_metrics as U

pytestmark = pytest.mark.gpu
FLOOR = 2e-6
# OBSERVED (MI355X): depth map form 2.8e-07, volume form 2.3e-07 (both at 7x13; 4.5e-08 at 36x48), at most 0.14 of the bound;
# the largest |seq32 - f64| / |f64| of the fixture is 6.4e-07 (36x48)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(dev):
    """name -> (device inputs, d_candi, fixture arrays): built once, shared, never written."""
    g = golden("g25_depth_metrics.npz")
    out = {}
    for name, (D, H, W) in U.CASES.items():
        inp = {k: torch.from_numpy(v).to(dev) for k, v in U.make_case(name).items()}
        out[name] = (inp, U.d_candi(D), {k: g[f"{name}_{k}"] for k in ("f64", "seq32", "n")})
    return out


def _check(got, count, fx, what):
    got, count = got.double().cpu().numpy(), count.cpu().numpy()
    f64, seq = fx["f64"], fx["seq32"].astype(np.float64)
    err = np.abs(got - f64)
    bound = np.maximum(np.abs(seq - f64), FLOOR * np.abs(f64))
    print(what, "max |hip - f64| / |f64| =", float((err / np.abs(f64)).max()), "max |seq32 - f64| / |f64| =",
          float((np.abs(seq - f64) / np.abs(f64)).max()), "worst err / bound =", float((err / bound).max()))
    assert np.array_equal(count, fx["n"].astype(np.float32)), (what, count, fx["n"])
    assert (err <= bound).all(), (what, (err / bound).max())


@pytest.mark.parametrize("name", list(U.CASES))
def test_both_forms_against_float64(cases, name):
    inp, dc, fx = cases[name]
    m, c, depth = ops.depth_metrics(inp["truth"], pred=inp["pred"], mask=inp["mask"], clamp_max=dc[-1])
    assert m.shape == (U.B, 9) and c.shape == (U.B,) and depth is None
    _check(m, c, fx, f"{name} depth map form")
    m, c, depth = ops.depth_metrics(inp["truth"], logp=inp["logp"], d_candi=dc, mask=inp["mask"], clamp_max=dc[-1])
    assert depth is None
    _check(m, c, fx, f"{name} volume form")
    m3, c3, _ = ops.depth_metrics(inp["truth"], pred=inp["pred"], mask=inp["mask"][:, 0], clamp_max=dc[-1])   # [B,H,W] mask
    assert torch.equal(m3, ops.depth_metrics(inp["truth"], pred=inp["pred"], mask=inp["mask"], clamp_max=dc[-1])[0])


@pytest.mark.parametrize("name", list(U.CASES))
def test_volume_form_depth_map_and_reproducibility(cases, name):
    inp, dc, _ = cases[name]
    kw = dict(mask=inp["mask"], clamp_max=dc[-1])
    m, c, depth = ops.depth_metrics(inp["truth"], logp=inp["logp"], d_candi=dc, want_depth=True, **kw)
    assert torch.equal(depth, ops.dpv_expect(inp["logp"], dc, BV_log=True))
    m0, c0, _ = ops.depth_metrics(inp["truth"], logp=inp["logp"], d_candi=dc, **kw)     # without the map: the same numbers
    assert torch.equal(m, m0) and torch.equal(c, c0)
    mp, cp, _ = ops.depth_metrics(inp["truth"], pred=depth, **kw)                          # the map form on that map: the same bits
    assert torch.equal(m, mp) and torch.equal(c, cp)
    for _ in range(2):
        m2, c2, d2 = ops.depth_metrics(inp["truth"], logp=inp["logp"], d_candi=dc, want_depth=True, **kw)
        assert torch.equal(m, m2) and torch.equal(c, c2) and torch.equal(depth, d2)
    assert torch.equal(mp, ops.depth_metrics(inp["truth"], pred=depth, **kw)[0])


def test_unaligned_volume_takes_the_any_shape_kernel(cases, dev):
    """A volume that does not start on a 16-byte boundary: the same values, and still dpv_expect's bits (both fall back alike)."""
    inp, dc, fx = cases["9x12"]
    flat = torch.empty(inp["logp"].numel() + 1, device=dev)
    logp = flat[1:].view_as(inp["logp"])
    logp.copy_(inp["logp"])
    assert logp.data_ptr() % 16 == 4 and logp.is_contiguous()
    m, c, depth = ops.depth_metrics(inp["truth"], logp=logp, d_candi=dc, mask=inp["mask"], clamp_max=dc[-1], want_depth=True)
    _check(m, c, fx, "9x12 unaligned volume")
    assert torch.equal(depth, ops.dpv_expect(logp, dc, BV_log=True))


def _one(dev, pred, truth, mask=None, clamp_max=None):
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float32, device=dev)   # noqa: E731
    m, c, _ = ops.depth_metrics(t(truth), pred=t(pred), mask=t(mask), clamp_max=clamp_max)
    return m.cpu().numpy(), c.cpu().numpy()


def _want(pred, truth, mask=None, clamp_max=None):
    rows = [U.metrics64(np.float32(p), np.float32(t), None if mask is None else np.float32(mask[b]), clamp_max)
            for b, (p, t) in enumerate(zip(pred, truth))]
    return np.stack([r[0] for r in rows]), np.asarray([r[1] for r in rows], dtype=np.float32)


def _close(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    np.testing.assert_allclose(got, want, rtol=FLOOR, atol=0, equal_nan=True)


def test_semantics(dev):
    pred = [[[8.0, 10.0, 12.0], [20.0, 30.0, 6.0]], [[9.0, 7.0, 14.0], [25.0, 11.0, 5.5]]]
    truth = [[[9.0, 9.5, 15.0], [18.0, 33.0, 7.0]], [[8.0, 7.5, 12.0], [28.0, 10.0, 6.5]]]
    base, n = _one(dev, pred, truth)
    _close(base, _want(pred, truth)[0])
    assert n.tolist() == [6.0, 6.0]
    # a mask of 0 excludes a pixel: the same numbers as the map without it (its prediction set to 0)
    mask = [[[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]], [[1.0] * 3, [1.0] * 3]]
    got, n = _one(dev, pred, truth, mask=mask)
    _close(got, _want(pred, truth, mask=mask)[0])
    assert n.tolist() == [5.0, 6.0] and np.array_equal(got[1], base[1]) and not np.array_equal(got[0], base[0])
    # a prediction of exactly 0 and a NaN prediction are excluded -- both give what the mask gave
    for hole in (0.0, NAN):
        p2 = [[[8.0, hole, 12.0], [20.0, 30.0, 6.0]], pred[1]]
        got2, n2 = _one(dev, p2, truth)
        assert np.array_equal(got2, got) and n2.tolist() == [5.0, 6.0], hole
    # a negative prediction is no valid pixel either
    got2, n2 = _one(dev, [[[8.0, -3.0, 12.0], [20.0, 30.0, 6.0]], pred[1]], truth)
    assert np.array_equal(got2, got) and n2.tolist() == [5.0, 6.0]
    # a truth at or above clamp_max is clamped; without clamp_max it is not
    far = [[[9.0, 9.5, 55.0], [18.0, 40.0, 7.0]], truth[1]]
    clamped, _ = _one(dev, pred, far, clamp_max=40.0)
    _close(clamped, _want(pred, [[[9.0, 9.5, 40.0], [18.0, 40.0, 7.0]], truth[1]])[0])
    free, _ = _one(dev, pred, far)
    _close(free, _want(pred, far)[0])
    assert free[0, 0] > clamped[0, 0] and np.array_equal(free[1], clamped[1])
    # a valid pixel whose truth is 0: the truth becomes -1, the log metrics of that item are NaN, the others are numbers
    zero_t = [[[9.0, 0.0, 15.0], [18.0, 33.0, 7.0]], truth[1]]
    got, n = _one(dev, pred, zero_t)
    want, _ = _want(pred, zero_t)
    _close(got, want)
    assert np.isnan(got[0, 4:7]).all() and np.isfinite(got[0, [0, 1, 2, 3, 7, 8]]).all() and n.tolist() == [6.0, 6.0]
    assert abs(got[0, 0] - (1 + 11 + 3 + 2 + 3 + 1) / 6) < 1e-6          # |10 - (-1)| = 11
    assert np.array_equal(got[1], base[1])
    # an item without a valid pixel: nine NaNs and count 0, its neighbour untouched
    got, n = _one(dev, pred, truth, mask=[[[0.0] * 3, [0.0] * 3], [[1.0] * 3, [1.0] * 3]])
    assert np.isnan(got[0]).all() and n.tolist() == [0.0, 6.0] and np.array_equal(got[1], base[1])
    # the argument order: the relative errors divide by the prediction, so swapping the maps changes them (and not the mae)
    swapped, _ = _one(dev, truth, pred)
    assert np.array_equal(swapped[:, 0], base[:, 0]) and np.array_equal(swapped[:, 1], base[:, 1])
    assert (np.abs(swapped[:, 7] - base[:, 7]) > 1e-3 * base[:, 7]).all()
    p, t = np.float64(pred[0]), np.float64(truth[0])
    assert abs(base[0, 7] - (np.abs(p - t) / p).mean()) < 1e-6 and abs(swapped[0, 7] - (np.abs(p - t) / t).mean()) < 1e-6
    # a fractional mask scales the prediction (the reference multiplies)
    got, _ = _one(dev, pred, truth, mask=[[[0.5] * 3, [0.5] * 3], [[1.0] * 3, [1.0] * 3]])
    _close(got, _want(pred, truth, mask=[np.full((2, 3), 0.5), np.ones((2, 3))])[0])


def test_depth_error_numpy_and_refusal(cases, dev):
    inp, dc, fx = cases["9x12"]
    masked = inp["pred"] * inp["mask"][:, 0]                                             # (an unmasked pixel with a zero truth is a NaN)
    m, c, _ = ops.depth_metrics(inp["truth"], pred=masked)
    assert bool(torch.isfinite(m).all())
    for b in range(U.B):
        row = img_utils.depth_error(masked[b].cpu().numpy(), inp["truth"][b].cpu().numpy())
        assert isinstance(row, list) and len(row) == 9 and all(isinstance(v, float) for v in row)
        assert row == m[b].tolist()
        assert img_utils.depth_error(masked[b], inp["truth"][b]) == row                  # device tensors
    # the evaluation loop's call: the masked prediction and the clamped truth as numpy maps -> the fixture's item
    p = (inp["pred"] * inp["mask"][:, 0]).cpu().numpy()
    t = inp["truth"].clone()
    t[t >= dc[-1]] = dc[-1]
    row = np.asarray(img_utils.depth_error(p[0], t[0].cpu().numpy()))
    assert (np.abs(row - fx["f64"][0]) <= np.maximum(np.abs(fx["seq32"][0] - fx["f64"][0]), FLOOR * fx["f64"][0])).all()
    with pytest.raises(RuntimeError, match="no valid pixel"):
        img_utils.depth_error(np.zeros((4, 5), np.float32), np.ones((4, 5), np.float32))
    with pytest.raises(RuntimeError, match="one size"):
        img_utils.depth_error(np.ones((4, 5), np.float32), np.ones((5, 4), np.float32))


def _frames(dev, seeds, B, H, W, D, with_labels):
    g = torch.Generator().manual_seed(77)
    frames = []
    for seed in seeds:
        inp = harness.move_input(synth.make_model_input(seed, B=B, V=1, H=H, W=W, D=D, pose="mono"), dev)
        coarse = 8.0 + 40.0 * torch.rand(B, 1, H // 16, W // 16, generator=g)          # up to 48 m: beyond the last candidate
        dmap = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        mask = (torch.rand(B, 1, H, W, generator=g) < 0.5).float()
        dmap = dmap * mask[:, 0]                                                        # 0 = no measurement
        gt = {"dmap_imgsizes": dmap.to(dev), "dmaps": dmap[:, ::4, ::4].contiguous().to(dev),
              "masks_imgsizes": mask.to(dev), "masks": mask[:, :, ::4, ::4].contiguous().to(dev)}
        if with_labels:
            K_up = inp["intrinsics"].clone()
            K_up[:, :2] *= 4.0
            inp["intrinsics_up"] = K_up
            gt["soft_labels_imgsize"] = [img_utils.gen_soft_label_torch(inp["d_candi"], gt["dmap_imgsizes"][b], torch.tensor(0.3, device=dev),
                                                                        zero_invalid=True) for b in range(B)]
        frames.append((inp, gt))
    return frames


def test_validate_runs_without_synchronising(dev):
    # 256 x 256: the smallest image BaseModel takes (its encoder pools 64 x 64 windows of the quarter-resolution features)
    B, H, W, D = 2, 256, 256, 64
    torch.manual_seed(0)
    model = get_model(synth.default_cfg("default"), 0)
    synth.seed_weights(model, seed=5)
    model = model.to(dev).eval()
    frames = _frames(dev, (9100, 9101), B, H, W, D, with_labels=True)
    cfg = synth.Cfg({"data": {"dataset_path": "/data/kitti"}})
    res = harness.validate(model, frames, cfg=cfg)                                      # (sets sync-debug "error" itself)
    assert torch.cuda.get_sync_debug_mode() == 0
    assert set(res) >= {"rmse", "rmse_refined", "sil", "sil_refined", "rmse_unc", "results", "results_refined"}
    assert tuple(res["results"]) == ops.DEPTH_METRIC_NAMES and len(res["steps"]) == 2
    clamp = float(frames[0][0]["d_candi"][-1])
    rows, rows_low, unc = [], [], []
    for (inp, gt), step in zip(frames, res["steps"]):
        assert step["depth_refined"].shape == (B, H, W) and step["depth_lowres"].shape == (B, H // 4, W // 4)
        assert step["errors"].shape == (B, 9) and step["rmse_unc"].shape == (B,)
        for b in range(B):
            for acc, depth, truth, mask in ((rows, step["depth_refined"], gt["dmap_imgsizes"], gt["masks_imgsizes"]),
                                            (rows_low, step["depth_lowres"], gt["dmaps"], gt["masks"])):
                t = truth[b].clone()
                t[t >= clamp] = clamp
                acc.append(img_utils.depth_error((depth[b] * mask[b, 0]).cpu().numpy(), t.cpu().numpy()))
            f_t, f_p, _ = img_utils.compute_unc_field(step["output"]["output_refined"][-1][b:b + 1], gt["soft_labels_imgsize"][b].unsqueeze(0),
                                                      inp["d_candi"], inp["intrinsics_up"][b:b + 1], gt["masks_imgsizes"][b], cfg)
            unc.append(float(img_utils.compute_unc_rmse(f_t, f_p, inp["d_candi"])))
    want, want_low = img_utils.eval_errors(rows), img_utils.eval_errors(rows_low)
    print("validate:", {k: res[k] for k in ("rmse", "rmse_refined", "sil", "sil_refined", "rmse_unc")}, "from depth_error:",
          want["rmse"][0], want_low["rmse"][0])
    assert np.isfinite(res["rmse_refined"]) and res["rmse_refined"] > 0
    assert abs(res["rmse_refined"] - want["rmse"][0]) <= 1e-6 * want["rmse"][0]
    assert abs(res["sil_refined"] - want["scale invariant log"][0]) <= 1e-6 * want["scale invariant log"][0]
    assert abs(res["rmse"] - want_low["rmse"][0]) <= 1e-6 * want_low["rmse"][0]
    assert abs(res["sil"] - want_low["scale invariant log"][0]) <= 1e-6 * want_low["scale invariant log"][0]
    assert res["results_refined"]["rmse"] == want["rmse"]
    np.testing.assert_allclose(res["rmse_unc"], float(np.mean(unc)), rtol=1e-6, equal_nan=True)
    # a model that leaves no depth maps behind takes the volume form: the same errors from one read of each volume
    class NoAux(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    res2 = harness.validate(NoAux(model), frames)
    assert res2["rmse_unc"] is None
    for k in ("rmse", "rmse_refined", "sil", "sil_refined"):
        assert abs(res2[k] - res[k]) <= 1e-6 * abs(res[k]), k
    assert torch.equal(res2["steps"][1]["depth_refined"], ops.dpv_expect(res2["steps"][1]["output"]["output_refined"][-1],
                                                                         frames[1][0]["d_candi"], BV_log=True))
