"""CPU suite of the range map and the occlusion masks: the float64 restatement the GPU tests compare against
(tests/util_occlusion.py) is checked against the reference's results (fixture g27_occlusion); the two torch compositions of
utils/warp_utils.py against the reference's; then the interface, and every refusal that is decided before a launch.

(The two loss functions have no CPU path -- their warp is the HIP inverse_warp -- so "occlusion=None returns what it returned
before" is checked on the GPU, bit for bit: tests/test_occlusion_gpu.py.)"""
import inspect

import numpy as np
import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.utils import warp_utils as wu
import util_occlusion as U


def _key(th):
    return str(th).replace("0.", "")


@pytest.mark.parametrize("name", U.DEPTH_CASES)
def test_depth_cases_against_the_restatement(name):
    """The chain and the splat in float64 against the reference's float64 run, 1e-12 (positions: of the largest one); the stored
    inputs are the builders'; both masks follow from the stored range maps; no pixel is within MARGIN of a threshold."""
    c = U.cases()[name]
    depth, Kinv, proj, holes, full = U.scene(name)
    assert np.array_equal(depth, c["depth"]) and np.array_equal(Kinv, c["Kinv"]) and np.array_equal(proj, c["proj"])
    assert tuple(depth.shape) == (2,) + U.SHAPES[name]
    if name == "c":
        assert np.array_equal(holes, c["holes"]) and np.array_equal(full, c["depth_full"]) and 0.05 < holes.mean() < 0.15
        assert not depth[holes == 1].any()
    pos = U.depth_positions(*(torch.from_numpy(v).double() for v in (depth, Kinv, proj)))
    ref = U.pos64(c)
    assert float((pos - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    r64 = U.range_map(pos)
    assert float((r64 - torch.from_numpy(c["r64"])).abs().max()) <= 1e-12
    e32 = float((torch.from_numpy(c["r32"]).double() - torch.from_numpy(c["r64"])).abs().max())
    assert e32 == float(c["e32"]) and 0 < e32 < 1e-4
    for tag, r in (("64", r64), ("32", torch.from_numpy(c["r32"]))):
        assert U.margin(r) > U.MARGIN
        for th in U.THS:
            assert np.array_equal(1 - c[f"occ{tag}_{_key(th)}"], U.visible(r, th).numpy())
    assert U.margin(U.range_map(torch.from_numpy(c["pos32"]).double())) > U.MARGIN
    for th in U.THS:   # float32 and float64 agree on every pixel: the margin at work
        assert np.array_equal(c[f"occ32_{_key(th)}"], c[f"occ64_{_key(th)}"])
    if name in ("b", "c"):   # positions leave the image on two sides
        H, W = U.SHAPES[name]
        x, y = torch.from_numpy(c["pos32"])[:, 0], torch.from_numpy(c["pos32"])[:, 1]
        assert bool((x > W - 1).any()) and bool((y < 0).any()) and bool((y > H - 1).any())
    if name != "d":
        assert 0.01 < c["occ64_2"].mean() < 0.12


@pytest.mark.parametrize("name", U.FLOW_CASES)
def test_flow_cases_against_the_restatement(name):
    """Dyadic weights: the restatement is exact in both precisions and equals the reference's range map bit for bit."""
    c = U.cases()[name]
    flow = U.flows(name)
    assert np.array_equal(flow, c["flow"], equal_nan=True)
    pos = U.base_grid(2, 16, 16) + torch.from_numpy(flow)
    r32, n = U.range_map(pos, want_count=True)
    r64 = U.range_map(pos.double())
    assert torch.equal(r32.double(), r64)
    if name == "e_nonfinite":
        bad = ~torch.isfinite(pos).all(1)
        assert 100 < int(bad.sum()) < 300 and bool(torch.isfinite(r64).all())
        live = torch.where(bad.unsqueeze(1), torch.full_like(pos, -5.0), pos)   # a non-finite position adds what a far one adds: nothing
        assert torch.equal(U.range_map(live.double()), r64)
        return
    assert np.array_equal(c["r32"], r32.numpy()) and np.array_equal(c["r64"], r64.numpy())
    for th in U.THS:
        assert np.array_equal(1 - c[f"occ64_{_key(th)}"], U.visible(r64, th).numpy())
        assert np.array_equal(c[f"occ32_{_key(th)}"], c[f"occ64_{_key(th)}"])
    if name == "e_int":
        assert np.array_equal(U.visible(r64, 0.2)[0, 0].numpy(), U.analytic_band())
        assert torch.equal(r64, r64.round()) and bool((n.double() >= r64).all())   # integer flows: r is an exact count
    if name == "e_collide":
        x, y = U.COLLIDE_AT
        assert float(r64[0, 0, y, x]) == 256.0 and float(r64.sum()) == 512.0
    if name == "e_edge":
        px, py = pos[:, 0], pos[:, 1]
        for v in (-1.0, 15.0, 16.0):
            assert bool((px == v).any()) and bool((py == v).any())


def test_flow_warp_and_bidirection_against_the_reference():
    c = U.cases()["flowpair"]
    x, f12, f21 = (torch.from_numpy(v) for v in U.flow_pair())
    assert np.array_equal(x.numpy(), c["x"]) and np.array_equal(f12.numpy(), c["flow12"]) and np.array_equal(f21.numpy(), c["flow21"])
    assert float((wu.flow_warp(x, f12) - torch.from_numpy(c["warp_border"])).abs().max()) <= 1e-6
    assert float((wu.flow_warp(x, f12, pad="zeros") - torch.from_numpy(c["warp_zeros"])).abs().max()) <= 1e-6
    assert float((wu.flow_warp(x, f12, "zeros", "nearest") - wu.flow_warp(x, f12, pad="zeros", mode="nearest")).abs().max()) == 0
    occ = wu.get_occu_mask_bidirection(f12, f21)
    assert occ.dtype == torch.float32 and tuple(occ.shape) == (2, 1, 16, 16)
    assert float((occ - torch.from_numpy(c["bidirection"]).float()).abs().max()) <= 1e-6
    assert 0.1 < float(occ.mean()) < 0.9
    grid = wu.mesh_grid(2, 3, 5)
    assert tuple(grid.shape) == (2, 2, 3, 5) and grid.dtype == torch.int64
    assert torch.equal(grid[1, 0], torch.arange(5).expand(3, 5)) and torch.equal(grid[0, 1], torch.arange(3).view(3, 1).expand(3, 5))
    n = wu.norm_grid(grid.float())
    assert tuple(n.shape) == (2, 3, 5, 2) and float(n.min()) == -1.0 and float(n.max()) == 1.0


def test_reference_signatures():
    def names(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]
    E = inspect.Parameter.empty
    assert names(wu.mesh_grid) == [("B", E), ("H", E), ("W", E)]
    assert names(wu.norm_grid) == [("v_grid", E)]
    assert names(wu.get_corresponding_map) == [("data", E)]
    assert names(wu.flow_warp) == [("x", E), ("flow12", E), ("pad", "border"), ("mode", "bilinear")]
    assert names(wu.get_occu_mask_bidirection) == [("flow12", E), ("flow21", E), ("scale", 0.01), ("bias", 0.5)]
    assert names(wu.get_occu_mask_backward) == [("flow21", E), ("th", 0.2)]
    assert names(ops.range_map) == [("coords", E)]
    assert names(ops.occlusion_mask) == [("coords", E), ("th", 0.2), ("want_range", False)]
    assert names(ops.depth_occlusion) == [("src_depth", E), ("Kinv", E), ("proj", E), ("th", 0.2), ("src_mask", None), ("want_range", False)]
    rsc = inspect.signature(lb.rgb_stereo_consistency_loss).parameters   # (a keyword, ahead of the mix's keywords whose places are pinned)
    assert list(rsc)[6:] == ["per_item", "occlusion", "ternary_weight", "ternary_md", "ssim_weight", "ssim_md", "fused"]
    dsc = inspect.signature(lb.depth_stereo_consistency_loss).parameters
    assert list(dsc)[-3:] == ["pose_src2target", "per_item", "occlusion"]
    assert rsc["occlusion"].default is None and dsc["occlusion"].default is None


def test_workspace_is_the_stated_formula():
    lib = _native.load()
    q = lib.pdepth_range_map_workspace_bytes
    for B, H, W in ((1, 1, 1), (2, 5, 7), (2, 21, 37), (4, 256, 512), (3, 4096, 4096)):
        assert q(B, H, W) == (8 * B * H * W + 255) // 256 * 256
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 4097, 4096), (65536, 4, 4)):
        assert q(*bad) == 0


def test_entries_refuse_before_any_launch():
    """Every validation path of the two entries, with its code and message; no GPU is touched (the pointers are never read)."""
    lib = _native.load()
    pos, dep = lib.pdepth_range_map_f32, lib.pdepth_depth_range_map_f32
    need = lib.pdepth_range_map_workspace_bytes(2, 8, 8)
    assert need == 1024
    nan = float("nan")

    def said(rc, code, words):
        return rc == code and words in lib.pdepth_last_error()

    def both(code, words, B=2, H=8, W=8, th=0.2, rng=512, vis=768, ws=1024, nbytes=need, only=None):
        got = []
        if only in (None, "pos"):
            got.append(said(pos(256, B, H, W, th, rng, vis, ws, nbytes, None), code, b"pdepth_range_map_f32: " + words))
        if only in (None, "dep"):
            got.append(said(dep(256, None, 256, 256, B, H, W, th, rng, vis, ws, nbytes, None), code, b"pdepth_depth_range_map_f32: " + words))
        return all(got)

    assert said(pos(None, 2, 8, 8, 0.2, 512, 768, 1024, need, None), 1, b"null pointer")
    for args in ((None, None, 256, 256), (256, None, None, 256), (256, 512, 256, None)):
        assert said(dep(*args, 2, 8, 8, 0.2, 512, 768, 1024, need, None), 1, b"null pointer")
    assert both(1, b"no output requested", rng=None, vis=None)
    for dims in (dict(B=0), dict(H=0), dict(W=-3)):
        assert both(1, b"non-positive dimension", **dims)
    assert both(1, b"H and W must be at least 2", H=1, only="dep")
    assert both(1, b"H*W must be at most 2^24 and B at most 65535", H=4097, W=4096)
    assert both(1, b"H*W must be at most 2^24 and B at most 65535", B=65536)
    assert both(1, b"th is NaN", th=nan)
    assert both(3, b"needs 1024 bytes of workspace (got 0); query pdepth_range_map_workspace_bytes()", ws=None, nbytes=0)
    assert both(3, b"needs 1024 bytes of workspace (got 1023)", nbytes=need - 1)
    assert both(3, b"workspace must be 256-byte aligned", ws=1024 + 64)
    # the order: arguments before the workspace
    assert both(1, b"th is NaN", th=nan, ws=None, nbytes=0)
    assert lib.pdepth_abi_version() == 6
    assert "csrc/occlusion.hip" in _native._SOURCE_OF_ENTRY.values()
    for name in ("pdepth_range_map_workspace_bytes", "pdepth_range_map_f32", "pdepth_depth_range_map_f32"):
        assert name in _native.EXPORTED_SYMBOLS and name in _native._ABSENT_FROM_EXPERIMENT_LIBS


def test_binding_refuses_before_any_launch():
    c = torch.zeros(2, 2, 8, 8)
    d, Ki, P = torch.ones(2, 8, 8), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3, 4)
    for call in (lambda: ops.range_map(c), lambda: ops.occlusion_mask(c), lambda: ops.occlusion_mask(c, 0.5, True),
                 lambda: ops.depth_occlusion(d, Ki, P), lambda: ops.depth_occlusion(d.clone().requires_grad_(True), Ki, P),
                 lambda: ops.depth_occlusion(d[:, None], Ki, P, src_mask=d[:, None]),
                 lambda: wu.get_corresponding_map(c), lambda: wu.get_occu_mask_backward(c)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(RuntimeError, match=r"coords must be \[B,2,H,W\].*\[2, 3, 8, 8\]"):
        ops.range_map(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match=r"coords must be \[B,2,H,W\].*\[2, 8, 8\]"):
        ops.occlusion_mask(torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError, match=r"coords must be \[B,2,H,W\]"):
        ops.range_map(torch.zeros(0, 2, 8, 8))
    with pytest.raises(RuntimeError, match="coords requires grad"):
        ops.range_map(c.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="coords requires grad"):
        ops.occlusion_mask(c.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        ops.range_map(c.numpy())
    with pytest.raises(TypeError, match="src_depth: expected a torch.Tensor"):
        ops.depth_occlusion(d.numpy(), Ki, P)
    with pytest.raises(RuntimeError, match=r"depth must be \[B,H,W\]"):
        ops.depth_occlusion(torch.ones(2, 3, 8, 8), Ki, P)
    with pytest.raises(RuntimeError, match=r"H, W >= 2"):
        ops.depth_occlusion(torch.ones(2, 1, 8), Ki, P)
    with pytest.raises(RuntimeError, match=r"Kinv must be \[2, 3, 3\]"):
        ops.depth_occlusion(d, Ki[:1], P)
    with pytest.raises(RuntimeError, match=r"proj must be \[2, 3, 4\]"):
        ops.depth_occlusion(d, Ki, torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match=r"src_mask must be \[2, 8, 8\]"):
        ops.depth_occlusion(d, Ki, P, src_mask=torch.ones(2, 8, 7))


def test_binding_refuses_other_dtypes():
    with pytest.raises(RuntimeError, match="coords: expected float32, got torch.float64"):
        ops.range_map(torch.zeros(2, 2, 8, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="depth: expected float32, got torch.float16"):
        ops.depth_occlusion(torch.ones(2, 8, 8, dtype=torch.float16), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="src_mask: expected float32, got torch.bool"):
        ops.depth_occlusion(torch.ones(2, 8, 8), torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3, 4), src_mask=torch.ones(2, 8, 8, dtype=torch.bool))


def test_loss_refuses_the_single_pass_op_with_an_occlusion_map():
    """fused=True is csrc/photo.hip, which has no mask input: refused before anything is computed."""
    z = torch.zeros(1, 3, 8, 8)
    for kw in ({}, {"ssim_weight": 0.85}):
        with pytest.raises(RuntimeError, match="no mask input"):
            lb.rgb_stereo_consistency_loss(z, z, z[:, 0], torch.eye(4)[None], torch.eye(3)[None], fused=True, occlusion=z[:, :1], **kw)
    with pytest.raises(RuntimeError, match="no census term"):   # the earlier refusal keeps its words
        lb.rgb_stereo_consistency_loss(z, z, z[:, 0], torch.eye(4)[None], torch.eye(3)[None], fused=True, ternary_weight=0.5)
