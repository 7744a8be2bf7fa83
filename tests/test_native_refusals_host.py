"""What the ctypes binding refuses before any launch, pinned word for word (fixture tests/golden/native_refusals.json, written by
tests/golden/make_native_refusals.py from the binding as it stood before its call path, workspace and tensor checks were folded).

For every public wrapper of _native that takes a tensor, WELL_FORMED holds one call on CPU tensors of the smallest legal shape and
the scalar refusals the wrapper has; cases() derives the rest mechanically: each tensor argument in turn replaced by a non-tensor,
by a float64 copy, by a tensor with its last dimension one larger, and by None, plus the well-formed call itself (CPU tensors: the
first device check refuses it).  Every case raises on a CPU; the fixture holds the exception's class name and its full message.

Callables of the module that are not in the table: NO_TENSOR (they take none).  None had to be left out for want of a GPU: every
wrapper judges the device of a tensor before it reaches the library."""
import inspect
import json
import os

import pytest
import torch

from pdepth_amd import _native

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_refusals.json")
NO_TENSOR = {"host_blas_mode": "answers from one CPU matmul", "load": "opens the library", "selected_kernel": "six integers in, a name out",
             "noncentred_guard": "reads the last workspace, takes sizes", "fallback_tiles": "reads the last workspace, takes sizes"}
UNREACHABLE_ON_CPU = {}   # callable -> why: none


def T(*shape, dtype=torch.float32):
    return torch.full(shape, 0.5, dtype=dtype)


def _cam(B=1, V=1, HW=16):
    return dict(K=T(B, 3, 3), R=T(B, V, 3, 3), t=T(B, V, 3), rays=T(B, 3, HW), cxcy=T(B, 2))


NAN = float("nan")
_VOL, _MAP, _DC, _IMG, _IMAP = (1, 4, 4, 4), (1, 4, 4), (4,), (1, 3, 7, 7), (1, 7, 7)
_GEO = dict(Kinv=T(1, 3, 3), proj=T(1, 3, 4))
_DSC = dict(src_depth=T(*_MAP), tgt_depth=T(*_MAP), src_mask=T(*_MAP), **_GEO, pose_row=T(1, 4), intr=T(1, 3, 3))
_RSC = dict(src_rgb=T(*_IMG), tgt_rgb=T(*_IMG), tgt_depth=T(*_IMAP), **_GEO)
_B1 = dict(count=T(1), g_value=T(1))
_XY = dict(x=T(*_IMG), y=T(*_IMG))
_FLOW = dict(x=T(*_IMG), flow=T(1, 2, 7, 7))
_CV = dict(x1=T(*_IMG), x2=T(*_IMG), flow=T(1, 2, 7, 7))
_FP = dict(im=T(*_IMG), other=T(*_IMG), flow=T(1, 2, 7, 7), mask=T(1, 1, 7, 7))
_FPW = dict(w_l1=0.15, w_ssim=0.85, w_ternary=1.0)
_LIDAR = dict(points=T(1, 8, 4), counts=torch.full((1,), 8, dtype=torch.int32), M_velo2cam=T(4, 4), intr=T(3, 4), height=8, width=8)
_CORR = dict(pad_size=1, kernel_size=1, max_displacement=1, stride1=1, stride2=1)

# wrapper -> (the well-formed call, {label: overrides} of its scalar refusals)
WELL_FORMED = {
    "pack_source": (dict(src=T(1, 1, 4, 4, 4)), {"src4d": dict(src=T(1, 4, 4, 4))}),
    "pack_views": (dict(feat=T(2, 4, 4, 4), rgb=T(2, 3, 8, 8), n_views=2), {"views3": dict(n_views=3), "rgb4ch": dict(rgb=T(2, 4, 8, 8))}),
    "sweep": (dict(ref=T(*_VOL), src=T(1, 1, 4, 4, 4), **_cam(), d_candi=T(*_DC), sigma=1.0), {"ref3d": dict(ref=T(4, 4, 4))}),
    "dpv_reduce": (dict(logits=T(*_VOL), d_candi=T(*_DC)), {"bf16": dict(logits=T(*_VOL, dtype=torch.bfloat16))}),
    "dpv_reduce_ex": (dict(logits=T(*_VOL), d_candi=T(*_DC), addend=T(*_VOL)),
                      {"prob_dtype": dict(prob_dtype=torch.float16), "bf16": dict(logits=T(*_VOL, dtype=torch.bfloat16))}),
    "ufield": (dict(dpv=T(*_VOL), d_candi=T(*_DC), intr=T(1, 3, 3), mask=T(*_MAP), bv_log=True, unc_ang=0.1, z_start=0.0, z_end=1.0,
                    min_depth=0.1, quash=True), {"no_mask": dict(mask=None)}),
    "dpv_expect": (dict(dpv=T(*_VOL), d_candi=T(*_DC), bv_log=True), {}),
    "dpv_moments": (dict(dpv=T(*_VOL), d_candi=T(*_DC)), {}),
    "warp_feature": (dict(src=T(1, 1, 4, 4, 4), **_cam(), d_candi=T(*_DC)), {}),
    "warp_feature_backward": (dict(g_out=T(1, 1, 4, 4, 4), **_cam(), d_candi=T(*_DC)), {"det": dict(deterministic=True)}),
    "sample_coords": (dict(**_cam(), d_candi=T(*_DC), H=4, W=4), {}),
    "dpv_fuse": (dict(logp=T(*_VOL), dmaps=T(*_MAP), masks=T(*_MAP), d_candi=T(*_DC), var=1.0, eps=1e-6), {}),
    "correlation_forward": (dict(x1=T(*_VOL), x2=T(*_VOL), **_CORR), {"grad": dict(x1=T(*_VOL).requires_grad_())}),
    "correlation_backward": (dict(x1=T(*_VOL), x2=T(*_VOL), grad_out=T(1, 9, 4, 4), **_CORR), {}),
    "inverse_warp": (dict(img=T(*_IMG), depth=T(*_IMAP), **_GEO), {"mode": dict(mode="cubic")}),
    "inverse_warp_backward": (dict(img=T(*_IMG), depth=T(*_IMAP), **_GEO, grad_out=T(*_IMG)), {"mode": dict(mode="cubic"), "det": dict(deterministic=True)}),
    "sweep_backward": (dict(ref=T(*_VOL), src=T(1, 1, 4, 4, 4), **_cam(), d_candi=T(*_DC), grad_cost=T(*_VOL), sigma=1.0),
                       {"no_output": dict(want_ref=False, want_src=False), "det": dict(deterministic=True)}),
    "dpv_reduce_backward": (dict(logp=T(*_VOL), d_candi=T(*_DC), g_logp=T(*_VOL), g_prob=T(*_VOL), g_depth=T(*_MAP)),
                            {"no_gradient": dict(g_logp=None, g_prob=None, g_depth=None)}),
    "dpv_reduce_backward_lp": (dict(logp=T(*_VOL), d_candi=T(*_DC), dtype=torch.bfloat16, g_logp=T(*_VOL), g_prob=T(*_VOL), g_depth=T(*_MAP)),
                               {"no_gradient": dict(g_logp=None, g_prob=None, g_depth=None), "dtype": dict(dtype=torch.float32)}),
    "dpv_expect_backward": (dict(dpv=T(*_VOL), d_candi=T(*_DC), bv_log=True, g_depth=T(*_MAP)), {}),
    "dpv_fuse_backward": (dict(logp=T(*_VOL), dmaps=T(*_MAP), masks=T(*_MAP), d_candi=T(*_DC), var=1.0, eps=1e-6, g_fused=T(*_VOL),
                               g_logfused=T(*_VOL)), {"no_gradient": dict(g_fused=None, g_logfused=None), "logp3d": dict(logp=T(4, 4, 4))}),
    "dpv_soft_ce": (dict(logp=T(*_VOL), d_candi=T(*_DC), label=T(*_VOL), mask=T(*_MAP)),
                    {"both": dict(depth_gt=T(*_MAP), variance=1.0), "neither": dict(label=None),
                     "depth_gt": dict(label=None, depth_gt=T(*_MAP), variance=1.0),
                     "no_variance": dict(label=None, depth_gt=T(*_MAP)), "variance0": dict(label=None, depth_gt=T(*_MAP), variance=0.0),
                     "varianceNaN": dict(label=None, depth_gt=T(*_MAP), variance=NAN)}),
    "dpv_soft_ce_backward": (dict(logp=T(*_VOL), d_candi=T(*_DC), count=T(1), label=T(*_VOL), mask=T(*_MAP), g_loss=T(1), g_depth=T(*_MAP)),
                             {"no_gradient": dict(g_loss=None, g_depth=None), "both": dict(depth_gt=T(*_MAP), variance=1.0)}),
    "loss_dsc": (dict(_DSC), {"pose_row1": dict(pose_row=T(2, 4))}),
    "loss_dsc_backward": (dict(_DSC, **_B1), {"det": dict(deterministic=True), "none": dict(want_src=False, want_tgt=False)}),
    "loss_rsc": (dict(_RSC), {"tiny": dict(tgt_depth=T(1, 1, 7))}),
    "loss_rsc_backward": (dict(_RSC, **_B1), {}),
    "loss_photo": (dict(_RSC, ssim_weight=0.85), {"md4": dict(md=4), "md0": dict(md=0), "window": dict(md=3, tgt_depth=T(1, 6, 7))}),
    "loss_photo_backward": (dict(_RSC, **_B1, ssim_weight=0.85), {"md4": dict(md=4), "window": dict(md=3, tgt_depth=T(1, 7, 6))}),
    "loss_dc": (dict(large=T(*_MAP), small=T(1, 1, 1)), {"least": dict(large=T(1, 3, 4))}),
    "loss_dc_backward": (dict(large=T(*_MAP), small=T(1, 1, 1), **_B1), {"least": dict(large=T(1, 4, 3))}),
    "loss_smooth": (dict(depth=T(*_MAP), rgb=T(1, 3, 4, 4)), {"least": dict(depth=T(1, 1, 4))}),
    "loss_smooth_backward": (dict(depth=T(*_MAP), rgb=T(1, 3, 4, 4), g_value=T(1)), {}),
    "ssim": (dict(_XY), {"md4": dict(md=4), "window": dict(md=3, x=T(1, 3, 6, 7), y=T(1, 3, 6, 7))}),
    "ssim_backward": (dict(_XY, g_out=T(1, 3, 5, 5)), {"md4": dict(md=4), "no_gradient": dict(want_x=False, want_y=False)}),
    "ternary": (dict(_XY), {"md4": dict(md=4), "patch": dict(md=3, x=T(1, 3, 6, 7), y=T(1, 3, 6, 7)), "grey": dict(x=T(1, 1, 7, 7), y=T(1, 1, 7, 7))}),
    "ternary_backward": (dict(_XY, g_out=T(1, 1, 7, 7)), {"md4": dict(md=4), "no_gradient": dict(want_x=False, want_y=False)}),
    "range_map": (dict(coords=T(1, 2, 4, 4)), {"thNaN": dict(th=NAN), "no_output": dict(want_range=False), "channels": dict(coords=T(1, 3, 4, 4))}),
    "depth_range_map": (dict(depth=T(*_MAP), **_GEO, src_mask=T(*_MAP)), {"thNaN": dict(th=NAN), "no_output": dict(want_range=False),
                                                                         "no_mask": dict(src_mask=None)}),
    "flow_warp": (dict(_FLOW), {"pad": dict(pad="x"), "h1": dict(x=T(1, 3, 1, 7))}),
    "flow_warp_backward": (dict(_FLOW, grad_out=T(*_IMG)), {"pad": dict(pad="x"), "no_gradient": dict(want_x=False, want_flow=False),
                                                            "det": dict(deterministic=True)}),
    "flow_fb_check": (dict(flow12=T(1, 2, 7, 7), flow21=T(1, 2, 7, 7)), {"channels": dict(flow12=T(1, 3, 7, 7))}),
    "flow_cost_volume": (dict(_CV), {"pad": dict(pad="x"), "md5": dict(max_displacement=5), "md1.5": dict(max_displacement=1.5),
                                     "slope-1": dict(negative_slope=-1.0), "slopeNaN": dict(negative_slope=NAN), "no_flow": dict(flow=None),
                                     "h1": dict(x1=T(1, 3, 1, 7), x2=T(1, 3, 1, 7))}),
    "flow_cost_volume_backward": (dict(_CV, out=T(1, 81, 7, 7), grad_out=T(1, 81, 7, 7)),
                                  {"pad": dict(pad="x"), "md0": dict(max_displacement=0), "det": dict(deterministic=True),
                                   "no_gradient": dict(want_x1=False, want_x2=False, want_flow=False)}),
    "flow_photo": (dict(_FP, **_FPW), {"pad": dict(pad="x"), "h2": dict(im=T(1, 3, 2, 7)), "h1": dict(im=T(1, 3, 1, 7)), "grey": dict(im=T(1, 1, 7, 7))}),
    "flow_photo_backward": (dict(_FP, **_B1, **_FPW), {"pad": dict(pad="x"), "count2": dict(count=T(2))}),
    "loss_smooth1": (dict(flo=T(1, 2, 7, 7), image=T(*_IMG), alpha=10.0), {"h1": dict(flo=T(1, 2, 1, 7), image=T(1, 3, 1, 7))}),
    "loss_smooth1_backward": (dict(flo=T(1, 2, 7, 7), image=T(*_IMG), alpha=10.0, g_value=T(1)), {"g_value2": dict(g_value=T(2))}),
    "depth_metrics": (dict(truth=T(*_MAP), logp=T(*_VOL), d_candi=T(*_DC), mask=T(*_MAP)),
                      {"both": dict(pred=T(*_MAP)), "neither": dict(logp=None), "pred": dict(logp=None, pred=T(*_MAP)),
                       "pred_want_depth": dict(logp=None, pred=T(*_MAP), want_depth=True), "truth4d": dict(truth=T(*_VOL))}),
    "flow_metrics": (dict(gt=T(1, 4, 4, 4), pred=T(1, 2, 2, 2), move_mask=T(*_MAP)), {"mask_on_2ch": dict(gt=T(1, 2, 4, 4)), "gt3ch": dict(gt=T(1, 3, 4, 4))}),
    "flow_resize": (dict(flow=T(1, 2, 2, 2), size=(4, 4)), {"channels": dict(flow=T(1, 3, 2, 2))}),
    "lidar_depth": (dict(_LIDAR), {"xyz5": dict(points=T(1, 8, 5)), "M1d": dict(M_velo2cam=T(4)), "batched": dict(M_velo2cam=T(1, 4, 4), intr=T(1, 3, 4)),
                                   "counts_i64": dict(counts=torch.full((1,), 8, dtype=torch.int64))}),
}


def _mutations(t):
    wider = tuple(t.shape[:-1]) + (t.shape[-1] + 1,)
    return {"nontensor": 3, "float64": t.double(), "dim+1": torch.full(wider, 0.5, dtype=t.dtype), "None": None}


def cases():
    """{case id: (wrapper name, kwargs)}: per wrapper the well-formed call, every mutation of every tensor argument, its scalars."""
    out = {}
    for fn, (base, scalars) in WELL_FORMED.items():
        out[f"{fn}/wellformed"] = (fn, base)
        for arg, value in base.items():
            if isinstance(value, torch.Tensor):
                for label, bad in _mutations(value).items():
                    out[f"{fn}/{arg}={label}"] = (fn, dict(base, **{arg: bad}))
        for label, override in scalars.items():
            out[f"{fn}/{label}"] = (fn, dict(base, **override))
    return out


def refusal(fn, kwargs):
    """(class name, message) of what the wrapper raises; (None, None) if it returns."""
    try:
        getattr(_native, fn)(**kwargs)
    except Exception as e:   # noqa: BLE001  (whatever it is, its class and text are what is pinned)
        return type(e).__name__, str(e)
    return None, None


CASES = cases()


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_is_the_fixtures(pinned):
    assert set(CASES) == set(pinned) and len(CASES) > 600


def test_every_public_callable_that_takes_a_tensor_is_in_the_table():
    public = {n for n, f in vars(_native).items() if inspect.isfunction(f) and f.__module__ == _native.__name__ and not n.startswith("_")}
    assert public - set(NO_TENSOR) - set(UNREACHABLE_ON_CPU) == set(WELL_FORMED)
    assert set(NO_TENSOR) <= public and not UNREACHABLE_ON_CPU
    assert {cid.split("/")[0] for cid in CASES} == set(WELL_FORMED)


@pytest.mark.parametrize("fn", sorted(WELL_FORMED))
def test_refusals_word_for_word(fn, pinned):
    """Every case of one wrapper raises, on a CPU, the class and the full text the fixture holds."""
    mine = {cid: kw for cid, (f, kw) in CASES.items() if f == fn}
    assert len(mine) >= 5
    for cid, kw in mine.items():
        kind, text = refusal(fn, kw)
        assert kind is not None, f"{cid}: returned"
        assert {"type": kind, "message": text} == pinned[cid], cid
