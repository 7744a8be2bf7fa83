"""CPU suite of the fused consistency and smoothness terms: the float64 restatement of tests/util_loss_terms.py reproduces the
reference's own values of the four terms (fixture g24: blk_dc, blk_dsc, blk_rsc, blk_smooth on item 0 of the inputs of
tests/util_loss.py) -- the yardstick is validated before the GPU suite uses it --; the input maker's conditions hold; the new C
entries are declared, bound and exported within ABI 6 and refuse bad arguments before any launch (no GPU needed: every call below
returns before touching a pointer); the ops and BaseLoss refuse what they must before the device."""
import ctypes

import pytest
import torch

import pdepth_amd
from pdepth_amd import _native, ops
from pdepth_amd.losses import loss_blocks as lb
from pdepth_amd.losses.losses import BaseLoss
from util import golden
import util_loss as U
import util_loss_terms as LT

FAKE = 256   # a non-null, 256-byte aligned "device pointer": validation fails before any use of it
NEW = ("pdepth_loss_terms_workspace_bytes", "pdepth_loss_dsc_f32", "pdepth_loss_dsc_backward_f32", "pdepth_loss_rsc_f32",
       "pdepth_loss_rsc_backward_f32", "pdepth_loss_dc_f32", "pdepth_loss_dc_backward_f32", "pdepth_loss_smooth_f32",
       "pdepth_loss_smooth_backward_f32")


def test_restatement_reproduces_the_reference():
    g = golden("g24_loss.npz")
    t = {k: torch.from_numpy(v) for k, v in U.make_inputs().items()}
    dl, dr = t["dmap_left_hi"][0:1], t["dmap_right_hi"][0:1].clamp(max=40.0)
    K, T = t["K_hi"][0:1], t["T_left2right"]
    Kinv, proj, back = LT.camera_matrices(K, T, lb._inv3)
    row = back[:, 2]
    rgb_l, rgb_r = t["rgb_left"][0:1, 0], t["rgb_right"][0:1, 0]
    got = {"blk_dc": LT.dc64(dl, t["dmap_left_lo"][0:1])[0],
           "blk_dsc": LT.dsc64(dr, dl, t["mask_right_hi"][0:1, 0], Kinv, proj, row, K)[0],
           "blk_rsc": LT.rsc64(rgb_r, rgb_l, dl, Kinv, proj)[0],
           "blk_smooth": LT.smooth64(dl, rgb_l)}
    for k, v in got.items():
        want = float(g[k])
        print(k, float(v), "reference", want, "relative", abs(float(v) - want) / abs(want))
        assert v.dtype == torch.float64 and abs(float(v) - want) <= 1e-6 * abs(want), (k, float(v), want)


@pytest.mark.parametrize("shape", LT.SHAPES)
def test_maker_conditions(shape):
    inp = LT.make_inputs(*shape)
    B, H, W = shape
    again = LT.make_inputs(*shape)
    assert all(torch.equal(inp[k], again[k]) for k in inp if inp[k] is not None)
    assert inp["tgt_depth"].dtype == torch.float32 and 7.0 < float(inp["tgt_depth"].min()) and float(inp["tgt_depth"].max()) < 37.0
    assert 0.3 < float(inp["src_mask"].mean()) < 0.7 or H * W <= 16
    assert (inp["small"] is None) == (H < 4) and (inp["small"] is None or tuple(inp["small"].shape) == (B, H // 4, W // 4))
    # the restatement is differentiable where the kernels are
    Kinv, proj, back = LT.camera_matrices(inp["intr"], inp["T"], lb._inv3)
    row = back[:, 2]
    src, tgt = inp["src_depth"].double().requires_grad_(True), inp["tgt_depth"].double().requires_grad_(True)
    value, count = LT.dsc64(src, tgt, inp["src_mask"], Kinv, proj, row, inp["intr"])
    (value.sum() + LT.rsc64(inp["src_rgb"], inp["tgt_rgb"], tgt, Kinv, proj)[0].sum() + LT.smooth64(tgt, inp["tgt_rgb"]).sum()).backward()
    assert value.shape == (B,) and bool((count > 0).all()) and bool(torch.isfinite(tgt.grad).all()) and float(src.grad.abs().sum()) > 0


def test_new_symbols_declared_bound_exported_abi_unchanged():
    lib = _native.load()
    for sym in NEW:
        assert sym in _native.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert lib.pdepth_abi_version() == 6


def _call(name, *args):
    lib = _native.load()
    rc = getattr(lib, name)(*args)
    return rc, lib.pdepth_last_error().decode()


def _ws(B, H, W):
    return _native.load().pdepth_loss_terms_workspace_bytes(B, H, W)


def test_entries_refuse_bad_arguments():
    P = [FAKE * i for i in range(1, 12)]
    need = _ws(2, 64, 96)
    assert need >= 2 * 2 * (64 * 96 // 256) * 4 and need % 256 == 0
    assert _ws(0, 64, 96) == 0 and _ws(1, 4097, 4097) == 0

    def dsc(B=2, H=64, W=96, src=P[0], value=P[7], ws=P[9], ws_bytes=need):
        return _call("pdepth_loss_dsc_f32", src, P[1], P[2], P[3], P[4], P[5], 0, P[6], B, H, W, value, P[8], ws, ws_bytes, None)

    def rsc(B=2, H=64, W=96, src=P[0], count=P[6], ws=P[9], ws_bytes=need):
        return _call("pdepth_loss_rsc_f32", src, P[1], P[2], P[3], P[4], B, H, W, P[5], count, ws, ws_bytes, None)

    def dc(B=2, H=64, W=96, small=P[1], ws=P[9], ws_bytes=need):
        return _call("pdepth_loss_dc_f32", P[0], small, B, H, W, P[2], P[3], ws, ws_bytes, None)

    def smooth(B=2, H=64, W=96, rgb=P[1], ws=P[9], ws_bytes=need):
        return _call("pdepth_loss_smooth_f32", P[0], rgb, B, H, W, P[2], ws, ws_bytes, None)

    for name, fn, null in (("dsc", dsc, dict(src=None)), ("rsc", rsc, dict(src=None)), ("dc", dc, dict(small=None)),
                           ("smooth", smooth, dict(rgb=None))):
        who = f"pdepth_loss_{name}_f32"
        assert fn(**null) == (1, f"{who}: null pointer")
        rc, msg = fn(B=0)
        assert rc == 1 and msg == f"{who}: non-positive dimension"
        rc, msg = fn(B=65536)
        assert rc == 1 and "B at most 65535" in msg
        rc, msg = fn(H=4097, W=4097)
        assert rc == 1 and "H*W must be at most 2^24" in msg
        least = 4 if name == "dc" else 2
        for dims in (dict(H=least - 1), dict(W=least - 1)):
            rc, msg = fn(**dims)
            assert rc == 1 and f"at least {least}" in msg, (name, dims, msg)
        rc, msg = fn(ws_bytes=(_ws(2, 16, 24) if name == "dc" else need) - 1)
        assert rc == 3 and "workspace" in msg
        assert fn(ws=None)[0] == 3
        rc, msg = fn(ws=FAKE + 1)
        assert rc == 3 and "aligned" in msg
    assert dsc(value=None) == (1, "pdepth_loss_dsc_f32: null output pointer")
    assert rsc(count=None) == (1, "pdepth_loss_rsc_f32: null output pointer")
    # the backward entries
    rc, msg = _call("pdepth_loss_dsc_backward_f32", P[0], P[1], P[2], P[3], P[4], P[5], 0, P[6], P[7], P[8], 2, 64, 96, None, None, None)
    assert rc == 1 and "no gradient requested" in msg
    rc, msg = _call("pdepth_loss_dsc_backward_f32", P[0], P[1], P[2], P[3], P[4], P[5], 0, P[6], None, P[8], 2, 64, 96, P[9], None, None)
    assert rc == 1 and msg == "pdepth_loss_dsc_backward_f32: null pointer"
    rc, msg = _call("pdepth_loss_rsc_backward_f32", P[0], P[1], P[2], P[3], P[4], P[5], P[6], 2, 64, 96, None, None)
    assert rc == 1 and msg == "pdepth_loss_rsc_backward_f32: null pointer"
    rc, msg = _call("pdepth_loss_rsc_backward_f32", P[0], P[1], P[2], P[3], P[4], P[5], P[6], 2, 1, 96, P[7], None)
    assert rc == 1 and "at least 2" in msg
    rc, msg = _call("pdepth_loss_dc_backward_f32", P[0], P[1], P[2], P[3], 2, 64, 96, None, None, None)
    assert rc == 1 and "no gradient requested" in msg
    rc, msg = _call("pdepth_loss_dc_backward_f32", P[0], P[1], P[2], P[3], 2, 3, 96, P[4], None, None)
    assert rc == 1 and "at least 4" in msg
    rc, msg = _call("pdepth_loss_smooth_backward_f32", P[0], P[1], P[2], 2, 64, 96, None, None)
    assert rc == 1 and msg == "pdepth_loss_smooth_backward_f32: null pointer"
    rc, msg = _call("pdepth_loss_smooth_backward_f32", P[0], P[1], P[2], 70000, 64, 96, P[3], None)
    assert rc == 1 and "B at most 65535" in msg


def test_ops_refuse_before_the_device():
    d, rgb = torch.zeros(1, 8, 8), torch.zeros(1, 3, 8, 8)
    K, P, row = torch.eye(3)[None], torch.zeros(1, 3, 4), torch.zeros(1, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_consistency(d, torch.zeros(1, 2, 2))
    with pytest.raises(RuntimeError, match=r"small must be \[1, 2, 2\]"):
        ops.depth_consistency(d, torch.zeros(1, 2, 3))
    with pytest.raises(RuntimeError, match="H, W >= 4"):
        ops.depth_consistency(torch.zeros(1, 2, 8), torch.zeros(1, 0, 2))
    with pytest.raises(RuntimeError, match="loss_blocks.edge_aware_smoothness_loss"):
        ops.edge_aware_smoothness(d, torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_aware_smoothness(d, rgb)
    with pytest.raises(RuntimeError, match=r"src_rgb must be \[1, 3, 8, 8\]"):
        ops.rgb_stereo_consistency(torch.zeros(1, 3, 8, 9), rgb, d, K, P)
    with pytest.raises(RuntimeError, match=r"pose_row must be \[1, 4\]"):
        ops.depth_stereo_consistency(d, d, d, K, P, torch.zeros(1, 3), K)
    for name, call in (("src_mask", lambda x: ops.depth_stereo_consistency(d, d, x(d), K, P, row, K)),
                       ("Kinv", lambda x: ops.depth_stereo_consistency(d, d, d, x(K), P, row, K)),
                       ("proj", lambda x: ops.depth_stereo_consistency(d, d, d, K, x(P), row, K)),
                       ("pose_row", lambda x: ops.depth_stereo_consistency(d, d, d, K, P, x(row), K)),
                       ("intr", lambda x: ops.depth_stereo_consistency(d, d, d, K, P, row, x(K)))):
        with pytest.raises(RuntimeError, match=f"depth_stereo_consistency: {name} requires grad"):
            call(lambda t: t.clone().requires_grad_(True))
    for name, call in (("src_rgb", lambda x: ops.rgb_stereo_consistency(x(rgb), rgb, d, K, P)),
                       ("tgt_rgb", lambda x: ops.rgb_stereo_consistency(rgb, x(rgb), d, K, P)),
                       ("Kinv", lambda x: ops.rgb_stereo_consistency(rgb, rgb, d, x(K), P)),
                       ("proj", lambda x: ops.rgb_stereo_consistency(rgb, rgb, d, K, x(P)))):
        with pytest.raises(RuntimeError, match=f"rgb_stereo_consistency: {name} requires grad"):
            call(lambda t: t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="edge_aware_smoothness: rgb requires grad"):
        ops.edge_aware_smoothness(d, rgb.clone().requires_grad_(True))


def test_base_loss_argument():
    crit = BaseLoss(U.loss_cfg(), 0)
    assert crit.fused_terms is False and crit.labels_from_depth is False
    assert BaseLoss(U.loss_cfg(), 0, fused_terms=True).fused_terms is True
    assert BaseLoss(U.loss_cfg(), 0, True, True).labels_from_depth is True
