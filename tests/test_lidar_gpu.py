"""GPU suite of the LiDAR ground-truth path: ops.lidar_depth (csrc/lidar_depth.hip), utils.lidar.generate_depth and
harness.targets_from_lidar against the float64 restatement of tests/util_lidar.py.

There is no golden fixture from the reference's generate_depth (its extension needs Eigen and OpenCV, which are not available
where these tests run): the contract is its source, restated in util_lidar.  Acceptance per case, over every pixel of all four
outputs: the non-zero pattern equals the float64 restatement's exactly; every non-zero depth is within
4 eps32 (|m20 x| + |m21 y| + |m22 z| + |m23 w|) of the float64 cam.z of the winning point (the rounding of the four-term chain in
any order; for the quarter map the largest such bound of its 4x4 block); masks are exactly 0 or 1.  The inputs are built so that
no fp32 rounding can flip a decision: constructed points sit 0.25 .. 0.75 of a pixel inside their pixel, the random scan is pruned
by util_lidar.prune (tests/test_lidar_host.py checks the generator)."""
import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import harness, ops
from pdepth_amd.utils import lidar

import util_lidar as U

pytestmark = pytest.mark.gpu
H0, W0 = 37, 53
OUT = {"dmap": "dmap_imgsizes", "mask": "masks_imgsizes", "dmap_quarter": "dmaps", "mask_quarter": "masks"}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _batch(items, dev, pad=3, filler=None):
    """list of [n,4|3] arrays -> (points [B,Nmax,dim] fp32 with NaN (or `filler` rows) behind every item's count, counts [B])."""
    items = [np.asarray(p, np.float32) for p in items]
    dim = items[0].shape[1]
    nmax = max(len(p) for p in items) + pad
    pts = np.full((len(items), nmax, dim), NAN, np.float32)
    for b, p in enumerate(items):
        if filler is not None:
            pts[b, :len(filler)] = filler[:nmax]
        pts[b, :len(p)] = p
    counts = torch.tensor([len(p) for p in items], dtype=torch.int32)
    return torch.from_numpy(pts).to(dev), counts.to(dev)


def _per_item(a, b, nd):
    a = np.asarray(a)
    return a[b] if a.ndim == nd + 1 else a


def _check(out, items, M, intr, H, W, f, filterdiff=1.0, pool_default=1000.0):
    """Every pixel of the four outputs of every item against the float64 restatement -> the restatements."""
    B = len(items)
    assert out["dmap_imgsizes"].shape == (B, H, W) and out["masks_imgsizes"].shape == (B, 1, H, W)
    assert out["dmaps"].shape == (B, H // 4, W // 4) and out["masks"].shape == (B, 1, H // 4, W // 4)
    assert all(out[k].dtype == torch.float32 for k in OUT.values())
    refs = []
    for b in range(B):
        ref = U.reference(items[b], _per_item(M, b, 2), _per_item(intr, b, 2), H, W, f, filterdiff, pool_default)
        got = {k: out[name][b].reshape(ref[k].shape).cpu().numpy() for k, name in OUT.items()}
        for k in OUT:
            assert np.array_equal(got[k] != 0, ref[k] != 0), (b, k, np.argwhere((got[k] != 0) != (ref[k] != 0))[:8])
        for k, m in (("dmap", "mask"), ("dmap_quarter", "mask_quarter")):
            assert np.isin(got[m], (0.0, 1.0)).all() and np.array_equal(got[m] == 1, got[k] != 0), (b, m)
        err = np.abs(got["dmap"].astype(np.float64) - ref["dmap"])
        assert (err <= ref["tol"]).all(), (b, float((err - ref["tol"]).max()))
        if ref["dmap_quarter"].size:
            tol_q = ref["tol"][:H // 4 * 4, :W // 4 * 4].reshape(H // 4, 4, W // 4, 4).max(axis=(1, 3))
            err_q = np.abs(got["dmap_quarter"].astype(np.float64) - ref["dmap_quarter"])
            assert (err_q <= tol_q).all(), (b, float((err_q - tol_q).max()))
        refs.append(ref)
    return refs


def _at(M, intr, rows, cols, depths, off=0.5):
    """Points that land `off` of a pixel inside pixel (row, col): u_f - 0.5 = col + off."""
    rows, cols, depths = np.broadcast_arrays(np.asarray(rows, float), np.asarray(cols, float), np.asarray(depths, float))
    return U.back_project(M, intr, cols.ravel() + off + 0.5, rows.ravel() + off + 0.5, depths.ravel())


def _run(items, M, intr, H, W, f, dev, filterdiff=1.0, **kw):
    pts, counts = _batch(items, dev)
    out = ops.lidar_depth(pts, counts, torch.from_numpy(np.asarray(M, np.float32)).to(dev),
                          torch.from_numpy(np.asarray(intr, np.float32)).to(dev), W, H, filtering=f, filterdiff=filterdiff, **kw)
    return out, _check(out, items, M, intr, H, W, f, filterdiff, kw.get("pool_default", 1000.0))


def test_truncation_at_the_edges(dev):
    """u_f - 0.5 of -0.3 and -0.9 is column 0 (truncation toward zero, not floor), -1.1 is outside; the same for rows; the last
    column and row take points but are never shown, and a position beyond them does not wrap into the next row.  filtering 0 shows
    row 0 and column 0."""
    M, intr = U.calibration(H0, W0)
    left = U.back_project(M, intr, np.array([-0.3, -0.9, -1.1]) + 0.5, np.array([5, 9, 13]) + 1.0, [4.0, 5.0, 6.0])
    top = U.back_project(M, intr, np.array([20, 24, 28]) + 1.0, np.array([-0.3, -0.9, -1.1]) + 0.5, [4.5, 5.5, 6.5])
    right = U.back_project(M, intr, np.array([W0 - 0.5, W0 + 0.2, W0 - 1.4]) + 0.5, np.array([16, 17, 19]) + 1.0, [7.0, 7.0, 7.0])
    bottom = U.back_project(M, intr, np.array([30, 32, 34]) + 1.0, np.array([H0 - 0.5, H0 + 0.2, H0 - 1.4]) + 0.5, [8.0, 8.0, 8.0])
    item0 = np.concatenate([left, top])
    item1 = np.concatenate([right, bottom, left[:1]])
    _, refs = _run([item0, item1], M, intr, H0, W0, 0, dev)
    d0, d1 = refs[0]["dmap"], refs[1]["dmap"]
    assert d0[5, 0] != 0 and d0[9, 0] != 0 and d0[13].sum() == 0 and d0[0, 20] != 0 and d0[0, 24] != 0 and d0[:, 28].sum() == 0
    assert (d0 != 0).sum() == 4
    # column W-2 / row H-2 are the last shown; W-1 / H-1 hold a point in the z-buffer, nothing wraps into (18, 0)
    assert refs[1]["zbuf"][16, W0 - 1] != 0 and refs[1]["zbuf"][H0 - 1, 30] != 0 and d1[19, W0 - 2] != 0 and d1[H0 - 2, 34] != 0
    assert (d1 != 0).sum() == 3 and d1[18, 0] == 0


def test_depth_threshold_and_non_finite_points(dev):
    """cam.z of 0.1001 is kept, 0.0999 and a negative depth are not; a NaN or an infinity in any coordinate skips the point."""
    M, intr = U.calibration(H0, W0)
    pts = _at(M, intr, [8, 12, 16], [10, 20, 30], [0.1001, 0.0999, -3.0])
    good = _at(M, intr, [22, 22, 22, 22, 26], [10, 14, 18, 22, 26], 6.0)
    broken = good.copy()
    broken[0, 0], broken[1, 1], broken[2, 2], broken[3, 3] = NAN, np.inf, -np.inf, NAN
    item0 = np.concatenate([pts, broken])
    item1 = np.concatenate([good, pts[::-1]])
    _, refs = _run([item0, item1], M, intr, H0, W0, 0, dev)
    d0 = refs[0]["dmap"]
    assert abs(d0[8, 10] - 0.1001) < 1e-6 and d0[12, 20] == 0 and d0[16, 30] == 0
    assert d0[22].sum() == 0 and d0[26, 26] != 0 and (d0 != 0).sum() == 2 and (refs[1]["dmap"] != 0).sum() == 6


def test_several_points_per_pixel_with_ties(dev):
    M, intr = U.calibration(H0, W0)
    one = np.concatenate([_at(M, intr, 10, 10, d, off) for d, off in ((5.0, 0.3), (3.0, 0.7), (7.0, 0.5), (3.0, 0.7), (3.0, 0.7))])
    two = np.concatenate([_at(M, intr, 20, 30, d, 0.25 + 0.5 * (i % 2)) for i, d in enumerate((9.0, 9.0, 2.5, 11.0, 2.5, 4.0))])
    _, refs = _run([np.concatenate([one, two]), np.concatenate([two[::-1], one[::-1]])], M, intr, H0, W0, 2, dev)
    for r in refs:
        assert abs(r["dmap"][10, 10] - 3.0) < 1e-5 and abs(r["dmap"][20, 30] - 2.5) < 1e-5 and (r["dmap"] != 0).sum() == 2


@pytest.mark.parametrize("f", [0, 2, 4])
def test_filter(dev, f):
    """A pixel is cleared by a nearer pixel at distance exactly f and kept at f + 1; the difference just on either side of
    -filterdiff; a pixel is not rescued by the removal of its occluder (the window reads the z-buffer: in-place filtering in raster
    order would keep P).  filtering 0 has no neighbours: everything inside the border stays."""
    M, intr = U.calibration(H0, W0)
    n = max(f, 1)   # where the "inside the window" neighbour goes (filtering 0: beside the pixel, outside its 1x1 window)
    rows = [6, 6, 6, 6, 12, 12, 12, 12, 18, 18, 18, 24, 24]
    cols = [10, 10 + n, 30, 30 + f + 1, 10, 10 + n, 30, 30 + n, 10, 10 + n, 10 + 2 * n, 10 + n, 10]
    deps = [10, 5, 10, 5, 10, 8.999, 10, 9.001, 6, 8, 10, 10, 5]
    item0 = _at(M, intr, rows, cols, deps)
    item1 = _at(M, intr, rows[::-1], [c + 1 for c in cols[::-1]], deps[::-1], 0.3)   # the same scene, one column on, other order
    _, refs = _run([item0, item1], M, intr, H0, W0, f, dev)
    for s, r in enumerate(refs):
        d = r["dmap"]
        assert (r["zbuf"] != 0).sum() == len(rows)
        gone = f > 0
        assert (d[6, 10 + s] == 0) == gone and d[6, 10 + n + s] != 0            # cleared at distance f
        assert d[6, 30 + s] != 0 and d[6, 30 + f + 1 + s] != 0                   # kept at f + 1
        assert (d[12, 10 + s] == 0) == gone and d[12, 30 + s] != 0               # -1.001 clears, -0.999 does not
        assert d[18, 10 + s] != 0 and (d[18, 10 + n + s] == 0) == gone and (d[18, 10 + 2 * n + s] == 0) == gone   # O2, O, P
        assert (d[24, 10 + n + s] == 0) == gone                                 # the occluder on the left works too
    # filterdiff is a parameter: with 1.5 the -1.001 step stays, the -2 steps still clear
    out2, refs2 = _run([item0], M, intr, H0, W0, f, dev, filterdiff=1.5)
    assert refs2[0]["dmap"][12, 10] != 0 and (refs2[0]["dmap"][18, 10 + n] == 0) == (f > 0)


@pytest.mark.parametrize("f", [0, 2, 4])
def test_zeroed_border(dev, f):
    """A point in every pixel: exactly rows f .. H-f-2 and columns f .. W-f-2 are non-zero (f leading, f + 1 trailing)."""
    M, intr = U.calibration(H0, W0)
    yy, xx = np.mgrid[0:H0, 0:W0]
    full = _at(M, intr, yy.ravel(), xx.ravel(), 5.0 + 0.01 * ((yy + 2 * xx) % 7).ravel())
    out, refs = _run([full, full[::-1]], M, intr, H0, W0, f, dev)
    want = np.zeros((H0, W0), bool)
    want[f:H0 - f - 1, f:W0 - f - 1] = True
    for b in range(2):
        assert np.array_equal(out["dmap_imgsizes"][b].cpu().numpy() != 0, want)


@pytest.mark.parametrize("f,H,W", [(0, 1, 20), (2, 5, 20), (4, 9, 23), (2, 20, 5), (1, 6, 7), (0, 6, 7), (2, 6, 7)])
def test_small_images(dev, f, H, W):
    """Images with H <= 2 f + 1 (or W) come out all zero -- the filter's region is empty --, whatever lands in them; a 6x7 image
    has a 1x1 quarter map."""
    M, intr = U.calibration(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    full = _at(M, intr, yy.ravel(), xx.ravel(), 3.0 + 0.3 * ((3 * yy + xx) % 5).ravel())   # (steps of 0.3: none at -filterdiff)
    out, refs = _run([full, full[: len(full) // 2]], M, intr, H, W, f, dev)
    if H <= 2 * f + 1 or W <= 2 * f + 1:
        assert all(float(out[k].abs().sum()) == 0 for k in OUT.values()) and (refs[0]["zbuf"] != 0).all()
    else:
        assert out["dmaps"].shape == (2, 1, 1) and (f > 1 or (refs[0]["dmap"] != 0).any())


def test_pool_quirks(dev):
    """The quarter map: a block of zeros is 0; a lone depth of 1000 or 1500 beside empty pixels disappears (the lifted zeros win or
    tie and the block "equals the default"); a block full of 1500 stays; an ordinary block takes its minimum.  M is a pure axis
    permutation here, so cam.z is the point's x exactly (1000 must be 1000 in fp32 and in float64 alike)."""
    M = np.eye(4)
    M[:3, :3] = [[0, -1, 0], [0, 0, -1], [1, 0, 0]]
    intr = np.array([[30.0, 0, 26.5, 0], [0, 30.0, 18.5, 0], [0, 0, 1, 0]])
    yy, xx = np.mgrid[16:20, 24:28]
    pts = np.concatenate([_at(M, intr, 4, 4, 1000.0), _at(M, intr, [8, 9], [20, 22], [1000.0, 1500.0]), _at(M, intr, 13, 9, 1500.0),
                          _at(M, intr, yy.ravel(), xx.ravel(), 1500.0), _at(M, intr, [24, 26], [12, 14], [7.0, 3.0])])
    pts[:, 0] = [1000.0, 1000.0, 1500.0, 1500.0] + [1500.0] * 16 + [7.0, 3.0]   # (the solve's last digit must not decide a tie)
    out, refs = _run([pts, pts[::-1]], M, intr, H0, W0, 0, dev)
    for b, r in enumerate(refs):
        q = out["dmaps"][b].cpu().numpy()
        assert r["dmap"][4, 4] == 1000 and r["dmap"][9, 22] == 1500
        assert q[1, 1] == 0 and q[2, 5] == 0 and q[3, 2] == 0 and q[0, 0] == 0
        assert q[4, 6] == 1500 and q[6, 3] == 3 and (q != 0).sum() == 2
    # pool_default is a parameter: with 2000 the lone depths survive
    out, refs = _run([pts], M, intr, H0, W0, 0, dev, pool_default=2000.0)
    assert (out["dmaps"][0].cpu().numpy() != 0).sum() == 5


def test_counts_ignore_the_rows_behind_them(dev):
    """counts = [0, n]: item 0 is all zero although its rows hold good points and NaNs; item 1 ignores what follows row n."""
    M, intr = U.calibration(H0, W0)
    good = _at(M, intr, [8, 12, 16, 20, 24], [10, 20, 30, 40, 25], [4.0, 5.0, 6.0, 7.0, 8.0])
    filler = np.concatenate([good, np.full((2, 4), NAN), _at(M, intr, [28, 30], [11, 33], [2.0, 2.0])]).astype(np.float32)
    pts, counts = _batch([good[:0], good[:3]], dev, pad=6, filler=filler)
    assert counts.tolist() == [0, 3] and torch.isnan(pts[0]).any() and not torch.isnan(pts[1, 3]).any()
    out = ops.lidar_depth(pts, counts, torch.from_numpy(M).float().to(dev), torch.from_numpy(intr).float().to(dev), W0, H0, filtering=0)
    _check(out, [good[:0], good[:3]], M, intr, H0, W0, 0)
    assert all(float(out[k][0].abs().sum()) == 0 for k in OUT.values())
    assert int((out["dmap_imgsizes"][1] != 0).sum()) == 3


@pytest.fixture(scope="module")
def scan(dev):
    """The pruned random scan: B = 2, about 20 k points per item in front of the camera, 64x192, filtering 2 -- several points
    per pixel, so the atomic minimum is contended.  Built once, shared, never written."""
    H, W, f = 64, 192, 2
    items, M, intr = [], None, None
    for seed in (12, 15):
        pts, M, intr, stats = U.pruned_scan(seed, 20000, H, W, f, half_fov_deg=50.0)
        assert stats["removed_in_image"] <= 0.02 * stats["in_image"] and stats["in_image"] > 2 * 2500
        items.append(pts)
    pts, counts = _batch(items, dev)
    return {"items": items, "M": M, "intr": intr, "H": H, "W": W, "f": f, "pts": pts, "counts": counts,
            "Md": torch.from_numpy(M).to(dev), "Id": torch.from_numpy(intr).to(dev)}


@pytest.fixture(scope="module")
def scan_out(scan):
    return ops.lidar_depth(scan["pts"], scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"], filtering=scan["f"])


def test_pruned_random_scan(scan, scan_out):
    refs = _check(scan_out, scan["items"], scan["M"], scan["intr"], scan["H"], scan["W"], scan["f"])
    for r in refs:
        occupied, shown = int((r["zbuf"] != 0).sum()), int((r["dmap"] != 0).sum())
        print("occupied", occupied, "shown", shown, "quarter", int((r["dmap_quarter"] != 0).sum()))
        assert occupied > 2500 and 0 < shown < occupied


def test_order_independence_and_reproducibility(scan, scan_out, dev):
    again = ops.lidar_depth(scan["pts"], scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"], filtering=scan["f"])
    g = torch.Generator().manual_seed(3)
    shuffled = [p[torch.randperm(len(p), generator=g).numpy()] for p in scan["items"]]
    pts, counts = _batch(shuffled, dev)
    perm = ops.lidar_depth(pts, counts, scan["Md"], scan["Id"], scan["W"], scan["H"], filtering=scan["f"])
    for k in OUT.values():
        assert torch.equal(again[k], scan_out[k]) and torch.equal(perm[k], scan_out[k]), k


def test_matrix_and_point_forms(scan, scan_out, dev):
    """Per-item matrices that repeat the shared ones, 3x3 intrinsics (the fourth column is zero then), [B,N,3] points against
    [B,N,4] with w = 1: the same bits.  Matrices that differ per item: each item against its own restatement."""
    H, W, f = scan["H"], scan["W"], scan["f"]
    B = len(scan["items"])
    rep = ops.lidar_depth(scan["pts"], scan["counts"], scan["Md"].expand(B, 4, 4), scan["Id"].expand(B, 3, 4), W, H, filtering=f)
    for k in OUT.values():
        assert torch.equal(rep[k], scan_out[k]), k
    I3 = scan["Id"][:, :3].contiguous()
    I4 = torch.cat([I3, torch.zeros(3, 1, device=dev)], dim=1)
    a = ops.lidar_depth(scan["pts"], scan["counts"], scan["Md"], I4, W, H, filtering=f)
    b = ops.lidar_depth(scan["pts"][:, :, :3].contiguous(), scan["counts"], scan["Md"], I3.expand(B, 3, 3), W, H, filtering=f)
    for k in OUT.values():
        assert torch.equal(a[k], b[k]), k
    assert int((a["dmap_imgsizes"] != 0).sum()) > 1000
    # different calibrations per item (constructed points: each item is built for its own matrices)
    M0, i0 = U.calibration(H0, W0)
    M1, i1 = M0.copy(), i0.copy()
    M1[:3, 3] += [0.05, -0.02, 0.1]
    i1[0, 0] *= 1.1
    i1[1, 2] += 2.0
    rows, cols, deps = [6, 10, 14, 18, 22, 26], [8, 16, 24, 32, 40, 44], [3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    items = [_at(M0, i0, rows, cols, deps), _at(M1, i1, rows, cols, deps)]
    out, refs = _run(items, np.stack([M0, M1]), np.stack([i0, i1]), H0, W0, 1, dev)
    assert all((r["dmap"] != 0).sum() == 6 for r in refs)
    swapped = ops.lidar_depth(*_batch(items, dev), torch.from_numpy(np.stack([M1, M0])).float().to(dev),
                              torch.from_numpy(np.stack([i1, i0])).float().to(dev), W0, H0, filtering=1)
    assert not torch.equal(swapped["dmap_imgsizes"], out["dmap_imgsizes"])


def test_outputs_feed_depth_metrics(scan_out):
    """The consumers' view: ops.depth_metrics(truth = dmaps, pred = dmaps, mask = masks) counts the non-zero pixels of each item."""
    for maps, masks in (("dmaps", "masks"), ("dmap_imgsizes", "masks_imgsizes")):
        errs, count, _ = ops.depth_metrics(scan_out[maps], pred=scan_out[maps], mask=scan_out[masks])
        want = (scan_out[maps] != 0).flatten(1).sum(1).float()
        assert torch.equal(count, want) and float(count.min()) > 0
        assert float(errs[:, :2].abs().max()) == 0


def test_targets_from_lidar(scan, scan_out):
    t = harness.targets_from_lidar(scan["pts"], scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"])
    B, H, W = len(scan["items"]), scan["H"], scan["W"]
    assert set(t) == {"dmaps", "dmap_imgsizes", "masks", "masks_imgsizes"}
    assert t["dmap_imgsizes"].shape == (B, H, W) and t["masks_imgsizes"].shape == (B, 1, H, W)
    assert t["dmaps"].shape == (B, H // 4, W // 4) and t["masks"].shape == (B, 1, H // 4, W // 4)
    assert all(v.dtype == torch.float32 and v.is_cuda for v in t.values())
    for k in t:   # the loader's default parameters are filtering 2, no resampling: the shared call
        assert torch.equal(t[k], scan_out[k]), k
    t0 = harness.targets_from_lidar(scan["pts"], scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"],
                                    {"filtering": 0, "upsample": 0, "filterdiff": 1})
    assert int((t0["dmap_imgsizes"] != 0).sum()) > int((t["dmap_imgsizes"] != 0).sum())


def test_call_does_not_synchronise(scan, scan_out):
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.lidar_depth(scan["pts"], scan["counts"], scan["Md"], scan["Id"][:, :3], scan["W"], scan["H"], filtering=scan["f"])
        t = harness.targets_from_lidar(scan["pts"], scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(t["dmaps"], scan_out["dmaps"]) and out["dmaps"].shape == scan_out["dmaps"].shape


def test_call_is_capturable(scan, scan_out, dev):
    """Three launches on the stream, nothing allocated by the library: captured into a graph and replayed on new points in the
    captured buffer, the call gives the eager answer bit for bit (the z-buffer is cleared again by every replay)."""
    pts = scan["pts"].clone()
    run = lambda: ops.lidar_depth(pts, scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"], filtering=scan["f"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    for k in OUT.values():
        assert torch.equal(out[k], scan_out[k]), k
    pts.copy_(scan["pts"].flip(0))
    graph.replay()
    torch.cuda.synchronize()
    want = ops.lidar_depth(scan["pts"].flip(0).contiguous(), scan["counts"], scan["Md"], scan["Id"], scan["W"], scan["H"],
                           filtering=scan["f"])
    for k in OUT.values():
        assert torch.equal(out[k], want[k]), k


def test_generate_depth_numpy(scan, scan_out, dev):
    """The reference's per-scan signature on float64 numpy input equals the batched call, item by item; a device tensor gives a
    device tensor; an attribute dict serves as params."""
    class Params:
        filtering, upsample = 2, 0

    for b, pts in enumerate(scan["items"]):
        got = lidar.generate_depth(pts.astype(np.float64), scan["intr"].astype(np.float64), scan["M"].astype(np.float64),
                                   scan["W"], scan["H"], {"filtering": scan["f"], "upsample": 0})
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (scan["H"], scan["W"])
        assert np.array_equal(got, scan_out["dmap_imgsizes"][b].cpu().numpy())
    n = int(scan["counts"][0])
    t = lidar.generate_depth(scan["pts"][0, :n], scan["Id"], scan["Md"], scan["W"], scan["H"], Params())
    assert t.is_cuda and torch.equal(t, scan_out["dmap_imgsizes"][0])
