"""The stream contract of include/pdepth.h, lines 13-14 -- launches are asynchronous, no host synchronisation, nothing is allocated
-- checked the way a caller relies on it: a step is captured into a graph and replayed on new data in the captured buffers
(tests/test_graph_replay_gpu.py, tests/test_graph_replay_host.py).  The module imports without a GPU.

  check_replays      the protocol: two input sets A and B (B from another seed, its incoming gradients -- or, for a forward op, its
                     features -- times 2^5, so that the exponent the integer sums choose per item differs), a warm-up on a side
                     stream, one capture, the replays A, B, A, A, each compared with the eager step on fresh clones
  BITS, Atomic       the two kinds of rule: the same bits; or, for a gradient summed with float atomics, the bound that the op's own
                     GPU suite already asserts, through the callable of that suite (Atomic.source names it)
  CASES              one row per op and path: Case(name, make_inputs, step, rules)
  stream_entries     the entries of include/pdepth.h whose prototype takes `void *stream`
  Recorder           a proxy around what _native.load() returns that notes the C entries called

What a replay can get wrong that an eager call cannot: an accumulator or the header word of the per-item exponent left over from
the previous replay (the third replay, A after B), a clear that the graph orders differently or drops, a launch that went to the
NULL stream and is not in the graph at all, a value read back to the host during capture and frozen into the graph (the fourth
replay repeats the third: a replay that depends on its predecessor differs there).

No tolerance is defined here.  Where a rule needs a yardstick -- the float32 evaluation's own error against float64 -- it is computed
on the inputs of the replay with the functions of the op's util module, and the bound is formed by that module's rule."""
import importlib
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import pdepth_amd  # noqa: F401
from pdepth_amd import _native, ops, synth
from pdepth_amd.utils import inverse_warp as iv

from pdepth_amd.losses import loss_blocks as lb

import util_cost_volume as UC
import util_flow as UF
import util_flow_photo as UFP
import util_loss_terms as LT
import util_photo as UP
import util_ssim as US
import util_ternary as UT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pdepth.h")
GAIN = 2.0 ** 5          # what B's incoming gradients (or features) are multiplied by
ORDER = "ABAA"           # the replays
SIGMA = 10.0
BITS = "bits"
MAX_ELEMENTS = 1 << 20   # no tensor of a case is larger


# ---- the header --------------------------------------------------------------------------------------------------------------------------
def stream_entries(path=HEADER):
    """The names of the entries whose C prototype takes `void *stream`, in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    protos = re.findall(r"\b(pdepth_\w+)\s*\(([^;{]*?)\)\s*;", text)
    return tuple(name for name, args in protos if re.search(r"void\s*\*\s*stream\b", args))


class Recorder:
    """Stands where _native.load() keeps the library and notes every pdepth_* entry that is called through it."""

    def __init__(self, lib, seen):
        self.__dict__["_lib"], self.__dict__["_seen"] = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pdepth_"):
            return fn
        seen = self._seen

        def call(*args):
            seen.add(name)
            return fn(*args)
        return call


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------
class Atomic:
    """The rule of an output that float atomics sum.  det_step: the eager step with deterministic=True, whose result is the eager
    side of the comparison; source: 'module:attribute', the callable of an existing suite that states the bound; check(got, det, ref)
    -> [(what, figure, bound)], got and det on the device, ref = reference(cpu inputs), computed once per input set."""

    def __init__(self, source, det_step, reference, check):
        self.source, self.det_step, self.reference, self.check = source, det_step, reference, check

    def resolve(self):
        module, attr = self.source.split(":")
        return getattr(importlib.import_module(module), attr)


class Case:
    def __init__(self, name, make_inputs, step, rules=BITS):
        self.name, self.make_inputs, self.step, self.rules = name, make_inputs, step, rules

    def __repr__(self):
        return self.name


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    """torch.equal, or the same bit patterns (a NaN that both sides hold in one place)."""
    return a.shape == b.shape and a.dtype == b.dtype and (torch.equal(a, b) or torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))


def tensors_of(inp):
    return {k: v for k, v in inp.items() if isinstance(v, torch.Tensor)}


def scaled(inp):
    """The input set as B takes it: the tensors its '_scaled' entry names times 2^5 (exact in every format used here)."""
    return {k: (v * GAIN if k in inp.get("_scaled", ()) else v) for k, v in inp.items()}


def _rule_of(rules, name):
    return rules if not isinstance(rules, dict) else rules.get(name, BITS)


def check_replays(make_inputs, step, rule=BITS, log=print, tag=""):
    """Capture `step` and replay it on A, B, A, A (see the module's docstring); raises AssertionError naming the first replay that
    differs.  make_inputs(seed) -> dict of CPU tensors (and constants: host candidates, sizes) with '_scaled' naming the tensors B
    multiplies by 2^5; step(inputs on the device) -> dict of output tensors; rule: BITS, an Atomic, or a dict output -> rule."""
    dev = torch.device("cuda:0")
    sets = {"A": make_inputs(0), "B": scaled(make_inputs(1))}
    for inp in sets.values():
        assert all(v.numel() <= MAX_ELEMENTS for v in tensors_of(inp).values())

    def fresh(inp):
        return {k: (v.to(dev).clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}

    def eager(inp, fn):
        return {k: v.detach().clone() for k, v in fn(fresh(inp)).items()}

    want = {s: eager(inp, step) for s, inp in sets.items()}
    atomics = {n: _rule_of(rule, n) for n in want["A"] if isinstance(_rule_of(rule, n), Atomic)}
    det, refs = {}, {}
    for n, r in atomics.items():
        for s, inp in sets.items():
            if (id(r), s) not in det:
                det[(id(r), s)] = eager(inp, r.det_step)
                refs[(id(r), s)] = r.reference(inp)
    # A and B must be two different problems: more than half of the output elements differ.  An element that is exactly zero on
    # both sides is not counted either way: a gradient that is sparse by construction (the one pixel per 4 x 4 block that
    # depth_consistency's g_large reaches, the texels a nearest-neighbour scatter misses) cannot differ there, and says nothing
    # about the two problems; for a dense output the count is that of all its elements.
    differ = sum(int((want["A"][n] != want["B"][n]).sum()) for n in want["A"])
    total = sum(int(((want["A"][n] != 0) | (want["B"][n] != 0)).sum()) for n in want["A"])
    assert total > 0 and 2 * differ > total, "%s: the eager results of A and B differ in %d of %d elements only" % (tag, differ, total)
    assert all(v.numel() <= MAX_ELEMENTS for v in want["A"].values())

    static = fresh(sets["A"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static)
    ran, figures = [], []
    for i, s in enumerate(ORDER, 1):
        for k, v in tensors_of(sets[s]).items():
            static[k].copy_(v.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        for n, got in out.items():
            r = _rule_of(rule, n)
            where = "%s: replay %d (%s), output %s" % (tag, i, s, n)
            if isinstance(r, Atomic):
                for what, figure, bound in r.check(got.detach(), det[(id(r), s)][n], refs[(id(r), s)]):
                    figures.append((i, s, n, what, figure, bound))
                    log("%s: %s %.3e, bound %.3e (%s)" % (where, what, figure, bound, r.source))
                    assert figure <= bound, "%s: %s %.3e exceeds the bound %.3e of %s" % (where, what, figure, bound, r.source)
            else:
                assert same_bits(got.detach(), want[s][n]), "%s differs from the eager call: %d of %d elements, max |diff| %.3e" % (
                    where, int((got != want[s][n]).sum()), got.numel(),
                    float((got.double() - want[s][n].double()).abs().nan_to_num(nan=float("inf")).max()) if got.numel() else 0.0)
        ran.append("%d:%s" % (i, s))
    log("%s: replays %s equal the eager step; outputs %s; %d of the %d elements that are not zero in both differ between A and B"
        % (tag, " ".join(ran), ", ".join("%s [%s]" % (n, "atomic" if n in atomics else "bits") for n in out), differ, total))
    del graph
    return figures


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(9100 + seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _leaf(t):
    return t.detach().requires_grad_(True)


def _grads(outs, leaves, gs):
    """torch.autograd.grad of sum_i <outs_i, gs_i> with respect to the leaves (inside the captured region: the binding's saved
    tensors and its _native backward are on the captured path)."""
    return torch.autograd.grad(list(outs), list(leaves), [g.reshape(o.shape) for o, g in zip(outs, gs)])


def candidates(D):
    return synth.powerf(5.0, 40.0, D, 1.0)   # float64 numpy, on the host: ops.d_candi_tensor uploads it once


# sweep: the "C9" case of tests/test_sweep_backward_pin_gpu.py (config 74, V 2, C 9, D 16, 24 x 40) at B = 2
SWEEP_SHAPE = dict(B=2, V=2, C=9, D=16, H=24, W=40)
CAMERA = ("K", "R", "t", "rays", "cxcy")


def _batch(config, shape, seed, g_shape=None, scaled_keys=("ref", "src")):
    s = dict(shape)
    B = s.pop("B")
    b = synth.make_batch(config + 100 * seed, B, pose="mono", **s)
    out = {k: b[k] for k in ("ref", "src") + CAMERA}
    out["d_candi"] = b["d_candi"]
    if g_shape is not None:
        out["g"] = _randn(_gen(seed), *g_shape)
    out["_scaled"] = scaled_keys
    return out


def sweep_forward_inputs(seed):
    return _batch(74, SWEEP_SHAPE, seed)


def sweep_backward_inputs(seed):
    s = SWEEP_SHAPE
    return _batch(74, s, seed, (s["B"], s["D"], s["H"], s["W"]), ("g",))


def sweep_dpv_backward_inputs(seed):
    s = SWEEP_SHAPE
    out = sweep_backward_inputs(seed)
    out["g_depth"] = _randn(_gen(seed + 50), s["B"], s["H"], s["W"])
    out["_scaled"] = ("g", "g_depth")
    return out


def _cam(inp):
    return tuple(inp[k] for k in CAMERA)


def sweep_forward_step(metric, algo):
    def step(inp):
        cost, logp, depth = ops.sweep_dpv(inp["ref"], inp["src"], *_cam(inp), inp["d_candi"], SIGMA, feat_dist=metric, algo=algo, want_cost=True)
        return {"cost": cost, "logp": logp, "depth": depth}
    return step


def sweep_backward_step(metric, deterministic):
    def step(inp):
        ref, src = _leaf(inp["ref"]), _leaf(inp["src"])
        cost = ops.sweep_cost(ref, src, *_cam(inp), inp["d_candi"], SIGMA, feat_dist=metric, deterministic=deterministic)
        g_ref, g_src = _grads([cost], [ref, src], [inp["g"]])
        return {"cost": cost, "g_ref": g_ref, "g_src": g_src}
    return step


def sweep_dpv_backward_step(inp):
    ref, src = _leaf(inp["ref"]), _leaf(inp["src"])
    _, logp, depth = ops.sweep_dpv(ref, src, *_cam(inp), inp["d_candi"], SIGMA, deterministic=True)
    g_ref, g_src = _grads([logp, depth], [ref, src], [inp["g"], inp["g_depth"]])
    return {"logp": logp, "depth": depth, "g_ref": g_ref, "g_src": g_src}


def _sweep_batch(inp):
    return {k: inp[k] for k in ("ref", "src", "d_candi") + CAMERA}


def sweep_atomic(metric):
    """g_src of the float-atomic path: the max-norm rule of util_sweep_backward against float64 at the kernel's positions, max (|g -
    g64| - L1 allowance)+ <= 2 E_ref + eps32 max|g64| with E_ref the figure of torch's CPU float32 autograd, and the rule of
    tests/test_sweep_backward_pin_gpu.py between the two paths, element by element, against the eager deterministic result."""
    import util_sweep_backward as U

    def reference(inp):
        b = _sweep_batch(inp)
        x = U.exact64_grads(b, inp["g"], SIGMA, metric)
        _, s32 = U.oracle_grads(b, inp["g"], SIGMA, metric, torch.float32, "cpu")
        x["E_ref"] = U.max_err(s32, x, "src")
        return x

    def check(got, det, x):
        import test_sweep_backward_pin_gpu as P
        P._between_paths("captured atomic g_src against the eager integer sum, %s" % metric, got.cpu(), det.cpu(), x)
        limit = 2 * x["E_ref"] + U.EPS32 * float(x["g_src"].abs().max())
        return [("max-norm error against float64", U.max_err(got.cpu(), x, "src"), limit)]

    return Atomic("util_sweep_backward:max_err", sweep_backward_step(metric, True), reference, check)


def sweep_cost_entry_step(inp):
    """pdepth_sweep_cost_f32 has no caller in the binding (ops.sweep_cost goes through pdepth_sweep_dpv_f32 with cost alone): the
    entry is called here as _native.sweep calls its sibling."""
    import ctypes
    lib = _native.load()
    ref, src = inp["ref"], inp["src"]
    B, V, C, H, W = src.shape
    dc = ops.d_candi_tensor(inp["d_candi"], ref.device)
    cam, keep = _native._camera(*_cam(inp), B, V, H * W)
    desc = _native.SweepDesc(B, V, C, dc.numel(), H, W, _native.METRIC_L2, _native.ALGO_AUTO, _native.host_blas_mode(), SIGMA,
                             C * H * W, V * C * H * W, C * H * W)
    ws_bytes = lib.pdepth_sweep_workspace_bytes(ctypes.byref(desc))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=ref.device)
    cost = torch.empty((B, dc.numel(), H, W), dtype=torch.float32, device=ref.device)
    rc = lib.pdepth_sweep_cost_f32(ctypes.byref(desc), ctypes.byref(cam), ref.data_ptr(), src.data_ptr(), dc.data_ptr(), cost.data_ptr(),
                                   ws.data_ptr(), ws_bytes, _native._stream(ref.device))
    _native._check(rc, lib)
    del keep
    return {"cost": cost}


# the packing entries: the shape of __graft_entry__.smoke(), which the distance-form kernel takes
PACK_SHAPE = dict(B=2, V=1, C=67, D=64, H=32, W=64)


def pack_source_inputs(seed):
    return _batch(9, PACK_SHAPE, seed)


def pack_source_step(inp):
    packed = ops.pack_source(inp["src"], PACK_SHAPE["D"])
    cost, logp, depth = ops.sweep_dpv(inp["ref"], packed, *_cam(inp), inp["d_candi"], SIGMA, want_cost=True)
    return {"cost": cost, "logp": logp, "depth": depth}


def pack_views_inputs(seed):
    s = PACK_SHAPE
    out = _batch(9, s, seed)
    g = _gen(seed)
    V1 = s["V"] + 1
    out["feat"] = _randn(g, s["B"] * V1, s["C"] - 3, s["H"], s["W"])
    out["rgb"] = torch.rand(s["B"] * V1, 3, 4 * s["H"], 4 * s["W"], generator=g)
    del out["ref"], out["src"]
    out["_scaled"] = ("feat", "rgb")
    return out


def pack_views_step(inp):
    packed, ref = ops.pack_views(inp["feat"], inp["rgb"], PACK_SHAPE["V"] + 1, PACK_SHAPE["D"])
    _, logp, depth = ops.sweep_dpv(ref, packed, *_cam(inp), inp["d_candi"], SIGMA)
    return {"ref": ref, "logp": logp, "depth": depth}


# warp_feature and inverse_warp: B 2, C 5, D 8, 17 x 23 (391 pixels: two workgroups, the second ragged)
WARP_SHAPE = dict(B=2, V=2, C=8, D=8, H=17, W=23)
IW_SHAPE = (2, 5, 17, 23)


def warp_feature_inputs(seed):
    s = WARP_SHAPE
    return _batch(51, s, seed, (s["B"], s["V"], s["D"], s["H"], s["W"]), ("g",))


def warp_feature_step(deterministic):
    def step(inp):
        src = _leaf(inp["src"])
        out = ops.warp_feature(src, *_cam(inp), inp["d_candi"], differentiable=True, deterministic=deterministic)
        (g_src,) = _grads([out], [src], [inp["g"]])
        return {"out": out, "g_src": g_src}
    return step


def sample_coords_step(inp):
    ix, iy = ops.sample_coords(*_cam(inp), inp["d_candi"], WARP_SHAPE["H"], WARP_SHAPE["W"])
    return {"ix": ix, "iy": iy}


def warp_feature_atomic():
    """g_src of the float-atomic path: the per-texel bound of util_warp_backward, |g32 - g64| <= (4 + n) eps32 A and exactly 0 where
    A == 0, through its check()."""
    import util_warp_backward as WB
    import util_warps as UW

    def reference(inp):
        b = _sweep_batch(inp)
        pos = UW.oracle_positions(b)
        g64, A = WB.oracle_grads(b, pos, inp["g"])
        return {"g64": g64, "A": A, "bound": (4 + WB.tap_counts(*pos)) * WB.EPS32 * A}

    def check(got, det, ref):
        ratio = WB.check(got, ref, "captured atomic g_src of warp_feature")
        return [("worst error / bound against float64", ratio, 1.0)]

    return Atomic("util_warp_backward:check", warp_feature_step(True), reference, check)


def inverse_warp_inputs(mode):
    """The inputs of util_warps at IW_SHAPE with the two matrices of utils.inverse_warp.warp_with_matrices; the upstream gradient is
    zero off util_warps.stable_mask, as in every comparison of that suite with float64."""
    def make(seed):
        import test_det_scatter_gpu as TD
        import util_warps as UW
        B, C, H, W = IW_SHAPE
        c = UW._iw_inputs(6200 + seed, B, C, H, W)
        order = (0, 1) if seed == 0 else (2, 0)
        pose = UW._pose44(B, [UW._T3[i] for i in order], [UW._A3[i] for i in order])
        Kinv, proj = torch.inverse(c["K"].double()).float(), torch.matmul(c["K"], pose[:, :3])
        _, ix, iy, pz = TD._warp_torch(c["img"].double(), c["depth"], Kinv, proj, mode, torch.float64)
        M = UW.stable_mask(ix, iy, pz, H, W, mode)
        assert float(M.double().mean()) > 0.9
        return {"img": c["img"], "depth": c["depth"], "Kinv": Kinv, "proj": proj, "g": c["gout"] * M.unsqueeze(1), "_scaled": ("g",), "mode": mode}
    return make


def inverse_warp_step(mode, deterministic):
    def step(inp):
        img, depth = _leaf(inp["img"]), _leaf(inp["depth"])
        out, valid = iv.warp_with_matrices(img, depth, inp["Kinv"], inp["proj"], mode, deterministic=deterministic)
        g_img, g_depth = _grads([out], [img, depth], [inp["g"]])
        return {"out": out, "valid": valid, "g_img": g_img, "g_depth": g_depth}
    return step


def inverse_warp_atomic(mode):
    """g_img of the float-atomic path: the rule of tests/test_det_scatter_gpu.py::test_inverse_warp_many_to_one, max |g - g64| <=
    max(4 e_ref, 4 eps32 max|g64|) with e_ref the float32 evaluation of the same chain in torch (its _warp_torch)."""
    def reference(inp):
        import test_det_scatter_gpu as TD
        import util_warps as UW
        grads = []
        for dtype in (torch.float64, torch.float32):
            img = inp["img"].to(dtype).requires_grad_(True)
            out = TD._warp_torch(img, inp["depth"], inp["Kinv"], inp["proj"], mode, dtype)[0]
            (out * inp["g"].to(dtype)).sum().backward()
            grads.append(img.grad.double())
        e_ref, scale = float((grads[1] - grads[0]).abs().max()), float(grads[0].abs().max())
        return {"g64": grads[0], "bound": max(4 * e_ref, 4 * UW.EPS32 * scale)}

    def check(got, det, ref):
        apart = float((got - det).abs().max())
        return [("max |g_img - float64| (%.3e from the eager integer sum)" % apart, float((got.double().cpu() - ref["g64"]).abs().max()), ref["bound"])]

    return Atomic("test_det_scatter_gpu:_warp_torch", inverse_warp_step(mode, True), reference, check)


# the flow ops: util_cost_volume.CASES[1] = ((2, 3, 19, 27), md 4)
FLOW_SHAPE, FLOW_MD = UC.CASES[1][0], UC.CASES[1][1]
assert FLOW_SHAPE == (2, 3, 19, 27) and FLOW_SHAPE in UF.SHAPES and FLOW_SHAPE[:1] + FLOW_SHAPE[2:] in UF.FB_SHAPES


def flow_inputs(seed):
    """x1, x2 ~ N(0, 1), flow ~ N(0, 3 px) (the distributions of util_flow.warp_inputs and util_cost_volume.inputs), images in (0, 1),
    a mask at 70 %, the upstream gradients of the warp and of the cost volume."""
    B, C, H, W = FLOW_SHAPE
    g = _gen(seed)
    out = {"x1": _randn(g, B, C, H, W), "x2": _randn(g, B, C, H, W), "flow": 3.0 * _randn(g, B, 2, H, W),
           "g": _randn(g, B, C, H, W), "g_cv": _randn(g, B, (2 * FLOW_MD + 1) ** 2, H, W), "g_value": torch.rand(1, generator=g) + 0.5}
    for k, s in (("im", 1), ("other", 2)):
        out[k] = torch.from_numpy(UF.smooth_image(B, H, W, 9300 + 10 * seed + s))
    out["mask"] = (torch.rand(B, 1, H, W, generator=g) < 0.7).float()
    amp = 0.2 if seed == 0 else 3.0   # the forward-backward check: A's flows stay under its bias (occ mostly 0), B's do not (mostly 1)
    out["fb12"], out["fb21"] = amp * _randn(g, B, 2, H, W), amp * _randn(g, B, 2, H, W)
    out["_scaled"] = ("g", "g_cv", "g_value")
    return out


def flow_warp_step(pad, deterministic):
    def step(inp):
        x, flow = _leaf(inp["x2"]), _leaf(inp["flow"])
        out = ops.flow_warp(x, flow, pad=pad, deterministic=deterministic)
        g_x, g_flow = _grads([out], [x, flow], [inp["g"]])
        return {"out": out, "g_x": g_x, "g_flow": g_flow}
    return step


def flow_warp_atomic(pad):
    """grad_x of the float-atomic path against the eager integer sum: util_flow.tol(e_ref, max|grad_out|), e_ref the error of the
    float32 evaluation of util_flow.flow_warp_ref against its float64 one on these inputs
    (tests/test_flow_gpu.py::test_scatter_determinism)."""
    def reference(inp):
        grads = []
        for dtype in (torch.float64, torch.float32):
            x = inp["x2"].to(dtype).requires_grad_(True)
            (gx,) = torch.autograd.grad(UF.flow_warp_ref(x, inp["flow"].to(dtype), pad), x, inp["g"].to(dtype))
            grads.append(gx.double())
        return UF.tol(float((grads[1] - grads[0]).abs().max()), inp["g"].abs().max())

    def check(got, det, tol):
        return [("max |grad_x - eager integer sum|", float((got - det).abs().max()), tol)]

    return Atomic("util_flow:tol", flow_warp_step(pad, True), reference, check)


def cost_volume_step(with_flow, deterministic, pad="border"):
    def step(inp):
        leaves = [_leaf(inp["x1"]), _leaf(inp["x2"])] + ([_leaf(inp["flow"])] if with_flow else [])
        out = ops.flow_cost_volume(leaves[0], leaves[1], leaves[2] if with_flow else None, max_displacement=FLOW_MD,
                                   negative_slope=UC.SLOPE, pad=pad, deterministic=deterministic)
        grads = _grads([out], leaves, [inp["g_cv"]])
        return dict(zip(("out", "g_x1", "g_x2", "g_flow"), (out,) + tuple(grads)))
    return step


def cost_volume_atomic(pad="border"):
    """grad_x2 of the float-atomic path against the eager integer sum: the tol_g_x2 of util_cost_volume.reference -- util_flow.tol
    of the float32 yardstick's error with the scale max|grad_out| max|x1| -- formed as that function forms it, on these inputs
    (tests/test_cost_volume_gpu.py::test_backward_bits)."""
    def reference(inp):
        grads = []
        for dtype in (torch.float64, torch.float32):
            x2 = inp["x2"].to(dtype).requires_grad_(True)
            out = UC.cost_volume_ref(inp["x1"].to(dtype), x2, inp["flow"].to(dtype), FLOW_MD, pad)
            grads.append(torch.autograd.grad(out, x2, inp["g_cv"].to(dtype))[0].double())
        return UF.tol(float((grads[1] - grads[0]).abs().max()), float(inp["g_cv"].abs().max()) * float(inp["x1"].abs().max()))

    def check(got, det, tol):
        return [("max |grad_x2 - eager integer sum|", float((got - det).abs().max()), tol)]

    return Atomic("util_cost_volume:reference", cost_volume_step(True, True, pad), reference, check)


def flow_photo_step(inp):
    flow = _leaf(inp["flow"])
    value, count = ops.flow_photometric(inp["im"], inp["other"], flow, inp["mask"], *UFP.WEIGHTS[0])
    (g_flow,) = _grads([value], [flow], [inp["g_value"]])
    return {"value": value, "count": count, "g_flow": g_flow}


def fb_check_step(inp):
    return {"occ": ops.flow_fb_check(inp["fb12"], inp["fb21"])}


SMOOTH_ALPHA = UF.smooth_inputs()[2]


def smooth1_step(inp):
    flo = _leaf(inp["flow"])
    value = ops.smooth_grad_1st(flo, inp["im"], SMOOTH_ALPHA)
    (g,) = _grads([value], [flo], [inp["g_value"]])
    return {"value": value, "g_flo": g}


def flow_metrics_inputs(seed):
    """A four-channel truth at the spatial size of FLOW_SHAPE, a prediction at a coarser odd size, a move mask."""
    B, _, H, W = FLOW_SHAPE
    g = _gen(seed)
    gt = torch.cat([4.0 * _randn(g, B, 2, H, W), (torch.rand(B, 1, H, W, generator=g) < 0.8).float(),
                    (torch.rand(B, 1, H, W, generator=g) < 0.6).float()], 1)
    gt[:, 3] *= gt[:, 2]
    return {"gt": gt, "pred": _randn(g, B, 2, 7, 10), "move": (torch.rand(B, H, W, generator=g) < 0.5).float(), "_scaled": ("pred",)}


def flow_metrics_step(inp):
    errors, counts, up = ops.flow_metrics(inp["gt"], inp["pred"], move_mask=inp["move"], want_flow=True)
    return {"errors": errors, "counts": counts, "flow_up": up}


def flow_resize_step(inp):
    B, _, H, W = FLOW_SHAPE
    return {"cv2": ops.flow_resize(inp["pred"], (H, W)), "aligned": ops.flow_resize(inp["pred"], (H, W), align_corners=True)}


# the splats: 2 x 19 x 27; B's coordinates are A's rule shifted by 3.5 pixels
def splat_inputs(seed):
    B, _, H, W = FLOW_SHAPE
    g = _gen(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xs, ys]).unsqueeze(0) + 2.0 * _randn(g, B, 2, H, W) + 3.5 * seed
    t = LT.make_inputs(B, H, W, seed=100 + seed)
    Kinv, proj, _ = LT.camera_matrices(t["intr"], t["T"], lb._inv3)
    return {"coords": coords, "depth": t["src_depth"], "mask": t["src_mask"], "Kinv": Kinv, "proj": proj, "_scaled": ()}


def range_map_step(inp):
    return {"range": ops.range_map(inp["coords"])}


def occlusion_mask_step(inp):
    vis, rng = ops.occlusion_mask(inp["coords"], want_range=True)
    return {"visible": vis, "range": rng}


def depth_occlusion_step(inp):
    vis, rng = ops.depth_occlusion(inp["depth"], inp["Kinv"], inp["proj"], src_mask=inp["mask"], want_range=True)
    return {"visible": vis, "range": rng}


# the loss terms: the smallest entry of the module's SHAPES with B >= 2
def smallest(shapes):
    return min((s for s in shapes if s[0] >= 2), key=lambda s: int(np.prod(s)))


TERMS_SHAPE, PHOTO_SHAPE = smallest(LT.SHAPES), smallest(UP.SHAPES)


def terms_inputs(shape):
    def make(seed):
        t = LT.make_inputs(*shape, seed=100 + seed)
        Kinv, proj, back = LT.camera_matrices(t["intr"], t["T"], lb._inv3)
        g = _gen(seed)
        B = shape[0]
        out = {k: t[k] for k in ("src_depth", "tgt_depth", "src_mask", "small", "src_rgb", "tgt_rgb", "intr")}
        out.update(Kinv=Kinv, proj=proj, pose_row=back[:, 2].contiguous(), g_value=torch.rand(B, generator=g) + 0.5, T=t["T"].numpy(),
                   _scaled=("g_value",))
        return out
    return make


def dsc_step(deterministic):
    def step(inp):
        src, tgt = _leaf(inp["src_depth"]), _leaf(inp["tgt_depth"])
        value, count = ops.depth_stereo_consistency(src, tgt, inp["src_mask"], inp["Kinv"], inp["proj"], inp["pose_row"], inp["intr"],
                                                    deterministic=deterministic)
        g_src, g_tgt = _grads([value], [src, tgt], [inp["g_value"]])
        return {"value": value, "count": count, "g_src_depth": g_src, "g_tgt_depth": g_tgt}
    return step


def dsc_atomic():
    """g_src_depth of the float-atomic path: the criterion of tests/test_det_scatter_gpu.py::_assert_dsc -- the error against the
    float64 restatement of util_loss_terms at most 2 E_ref + 1e-6 of the largest gradient, E_ref the error of the float32
    composition of losses/loss_blocks.py -- through that function."""
    def reference(inp):
        import test_loss_terms_gpu as TL
        T = torch.from_numpy(inp["T"])
        sides = {}
        for name, fn, dtype, dev in (("g64", TL._restatement, torch.float64, "cpu"), ("comp", TL._composition, None, "cuda:0")):
            t = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
            t["back"], t["pose"] = torch.inverse(T).unsqueeze(0).to(dev), T.unsqueeze(0).to(dev)
            x = TL._leaves("dsc", t, dtype)
            value = fn("dsc", t, x)
            value = value[0] if isinstance(value, tuple) else value
            (value * t["g_value"].to(value.dtype)).sum().backward()
            sides[name] = {"src_depth": x["src_depth"].grad.detach()}
        return sides

    def check(got, det, ref):
        import test_det_scatter_gpu as TD
        TD._assert_dsc("captured atomic g_src_depth", {"src_depth": got}, ref["comp"], ref["g64"])
        big = float(ref["g64"]["src_depth"].abs().max())
        e_ref = float((ref["comp"]["src_depth"].double().cpu() - ref["g64"]["src_depth"]).abs().max())
        return [("max |g_src_depth - float64|", float((got.double().cpu() - ref["g64"]["src_depth"]).abs().max()), 2 * e_ref + 1e-6 * big)]

    return Atomic("test_det_scatter_gpu:_assert_dsc", dsc_step(True), reference, check)


def rsc_step(ssim_weight):
    def step(inp):
        tgt = _leaf(inp["tgt_depth"])
        value, count = ops.rgb_stereo_consistency(inp["src_rgb"], inp["tgt_rgb"], tgt, inp["Kinv"], inp["proj"], ssim_weight=ssim_weight)
        (g,) = _grads([value], [tgt], [inp["g_value"]])
        return {"value": value, "count": count, "g_tgt_depth": g}
    return step


def dc_step(inp):
    large, small = _leaf(inp["tgt_depth"]), _leaf(inp["small"])
    value, count = ops.depth_consistency(large, small)
    g_large, g_small = _grads([value], [large, small], [inp["g_value"]])
    return {"value": value, "count": count, "g_large": g_large, "g_small": g_small}


def smooth_step(inp):
    depth = _leaf(inp["tgt_depth"])
    value = ops.edge_aware_smoothness(depth, inp["tgt_rgb"])
    (g,) = _grads([value], [depth], [inp["g_value"]])
    return {"value": value, "g_depth": g}


assert US.SHAPE == UT.SHAPE and US.SHAPE[0] >= 2


def window_inputs(md):
    def make(seed):
        B, C, H, W = US.SHAPE
        g = _gen(seed)
        x = torch.from_numpy(UF.smooth_image(B, H, W, 9400 + seed)) + 0.02 * _randn(g, B, C, H, W)
        y = x + 0.1 * _randn(g, B, C, H, W)
        return {"x": x, "y": y, "g_ssim": _randn(g, B, C, H - 2 * md, W - 2 * md), "g_tern": _randn(g, B, 1, H, W), "_scaled": ("g_ssim", "g_tern")}
    return make


def window_step(op, md):
    def step(inp):
        x, y = _leaf(inp["x"]), _leaf(inp["y"])
        out = (ops.ssim if op == "ssim" else ops.ternary)(x, y, md)
        g_x, g_y = _grads([out], [x, y], [inp["g_ssim" if op == "ssim" else "g_tern"]])
        return {"out": out, "g_x": g_x, "g_y": g_y}
    return step


# the DPV reductions: 2 x 16 x 12 x 20, and 2 x 7 x 5 x 9 for the any-shape kernels
DPV_SHAPES = ((2, 16, 12, 20), (2, 7, 5, 9))


def dpv_inputs(shape, dtype=torch.float32):
    def make(seed):
        B, D, H, W = shape
        g = _gen(seed)
        logits, addend = 3.0 * _randn(g, B, D, H, W), _randn(g, B, D, H, W)
        logp = F.log_softmax(logits + addend, 1)
        dc = candidates(D)
        depth_gt = 5.0 + 35.0 * torch.rand(B, H, W, generator=g)
        return {"logits": logits.to(dtype), "addend": addend.to(dtype), "logp": logp, "prob": logp.exp(), "d_candi": dc,
                "g_logp": _randn(g, B, D, H, W), "g_prob": _randn(g, B, D, H, W), "g_depth": _randn(g, B, H, W), "g_loss": torch.rand(B, generator=g) + 0.5,
                "label": F.softmax(2.0 * _randn(g, B, D, H, W), 1), "depth_gt": depth_gt, "mask": (torch.rand(B, H, W, generator=g) < 0.6).float(),
                "pred": depth_gt * (1.0 + 0.2 * _randn(g, B, H, W)).clamp(0.3, 3.0),
                "intr": torch.tensor([[(0.9 + 0.05 * seed) * W, 0.0, W / 2.0 + 0.3], [0.0, (0.95 + 0.05 * seed) * H, H / 2.0 - 0.4], [0.0, 0.0, 1.0]]).repeat(B, 1, 1),
                "_scaled": ("g_logp", "g_prob", "g_depth", "g_loss")}
    return make


def dpv_reduce_step(inp):
    logits = _leaf(inp["logits"])
    logp, depth = ops.dpv_reduce(logits, inp["d_candi"])
    (g,) = _grads([logp, depth], [logits], [inp["g_logp"], inp["g_depth"]])
    return {"logp": logp, "depth": depth, "g_logits": g}


def dpv_reduce_nograd_step(inp):
    logp, depth = ops.dpv_reduce(inp["logits"], inp["d_candi"])
    return {"logp": logp, "depth": depth}


def dpv_reduce_ex_step(quarter=True):
    def step(inp):
        logits, addend = _leaf(inp["logits"]), _leaf(inp["addend"])
        out = ops.dpv_reduce_ex(logits, inp["d_candi"], addend=addend, want_logp=True, want_prob=True, want_depth=True, want_var=True,
                                want_quarter=quarter)
        g_logits, g_addend = _grads([out["logp"], out["prob"], out["depth"]], [logits, addend],
                                    [inp["g_logp"], inp["g_prob"].to(out["prob"].dtype), inp["g_depth"]])
        return dict(out, g_logits=g_logits, g_addend=g_addend)
    return step


def dpv_expect_step(bv_log):
    def step(inp):
        dpv = _leaf(inp["logp" if bv_log else "prob"])
        depth = ops.dpv_expect(dpv, inp["d_candi"], BV_log=bv_log)
        (g,) = _grads([depth], [dpv], [inp["g_depth"]])
        return {"depth": depth, "g_dpv": g}
    return step


def dpv_moments_step(inp):
    mean, var = ops.dpv_moments(inp["logp"], inp["d_candi"], BV_log=True)
    mean_p, var_p = ops.dpv_moments(inp["prob"], inp["d_candi"], BV_log=False)
    return {"mean": mean, "var": var, "mean_p": mean_p, "var_p": var_p}


def dpv_fuse_step(inp):
    logp = _leaf(inp["logp"])
    fused, logf = ops.dpv_fuse(logp, inp["depth_gt"], inp["mask"], inp["d_candi"])
    (g,) = _grads([fused, logf], [logp], [inp["g_prob"], inp["g_logp"]])
    return {"fused": fused, "log_fused": logf, "g_logp": g}


def soft_ce_step(form):
    def step(inp):
        logp = _leaf(inp["logp"])
        kw = {"label": inp["label"]} if form == "label" else {"depth_gt": inp["depth_gt"], "variance": 0.3}
        loss, depth = ops.dpv_soft_ce(logp, inp["d_candi"], mask=inp["mask"], want_depth=True, **kw)
        (g,) = _grads([loss, depth], [logp], [inp["g_loss"], inp["g_depth"]])
        return {"loss": loss, "depth": depth, "g_logp": g}
    return step


def ufield_step(inp):
    plane, dzero = ops.ufield(inp["logp"], inp["d_candi"], inp["intr"], mask=inp["mask"])
    return {"plane": plane, "depth_zero": dzero}


def depth_metrics_step(inp):
    m1, c1, _ = ops.depth_metrics(inp["depth_gt"], pred=inp["pred"], mask=inp["mask"], clamp_max=float(inp["d_candi"][-1]))
    m2, c2, depth = ops.depth_metrics(inp["depth_gt"], logp=inp["logp"], d_candi=inp["d_candi"], mask=inp["mask"], want_depth=True)
    return {"metrics_map": m1, "count_map": c1, "metrics_volume": m2, "count_volume": c2, "depth": depth}


# the correlation: (2, 9, 17, 35), md 4
CORR_SHAPE, CORR_MD = (2, 9, 17, 35), 4


def correlation_inputs(dtype):
    def make(seed):
        B, C, H, W = CORR_SHAPE
        g = _gen(seed)
        return {"x1": _randn(g, B, C, H, W).to(dtype), "x2": _randn(g, B, C, H, W).to(dtype),
                "g": (0.1 * _randn(g, B, (2 * CORR_MD + 1) ** 2, H, W)).to(dtype), "_scaled": ("g",)}
    return make


def correlation_step(inp):
    x1, x2 = _leaf(inp["x1"]), _leaf(inp["x2"])
    out = ops.correlation(x1, x2, pad_size=CORR_MD, kernel_size=1, max_displacement=CORR_MD, stride1=1, stride2=1)
    g1, g2 = _grads([out], [x1, x2], [inp["g"]])
    return {"out": out, "g_x1": g1, "g_x2": g2}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    for metric, algos in (("L2", ("direct", "tiled1", "dist", "auto")), ("L1", ("direct", "tiled1", "auto"))):   # (L1 has no distance form)
        for algo in algos:
            add("sweep_forward-%s-%s" % (metric, algo), sweep_forward_inputs, sweep_forward_step(metric, algo))
    for metric in ("L2", "L1"):
        add("sweep_backward-%s-atomic" % metric, sweep_backward_inputs, sweep_backward_step(metric, False), {"g_src": sweep_atomic(metric)})
        add("sweep_backward-%s-det" % metric, sweep_backward_inputs, sweep_backward_step(metric, True))
    add("sweep_dpv_backward-det", sweep_dpv_backward_inputs, sweep_dpv_backward_step)
    add("sweep_cost_entry", sweep_forward_inputs, sweep_cost_entry_step)
    add("pack_source-packed_sweep", pack_source_inputs, pack_source_step)
    add("pack_views-packed_sweep", pack_views_inputs, pack_views_step)
    add("warp_feature-atomic", warp_feature_inputs, warp_feature_step(False), {"g_src": warp_feature_atomic()})
    add("warp_feature-det", warp_feature_inputs, warp_feature_step(True))
    add("sample_coords", warp_feature_inputs, sample_coords_step)
    for mode in ("bilinear", "nearest"):
        add("inverse_warp-%s-atomic" % mode, inverse_warp_inputs(mode), inverse_warp_step(mode, False), {"g_img": inverse_warp_atomic(mode)})
        add("inverse_warp-%s-det" % mode, inverse_warp_inputs(mode), inverse_warp_step(mode, True))
    for pad in UF.PADS:
        add("flow_warp-%s-atomic" % pad, flow_inputs, flow_warp_step(pad, False), {"g_x": flow_warp_atomic(pad)})
        add("flow_warp-%s-det" % pad, flow_inputs, flow_warp_step(pad, True))
    add("flow_cost_volume-flow-atomic", flow_inputs, cost_volume_step(True, False), {"g_x2": cost_volume_atomic()})
    add("flow_cost_volume-flow-det", flow_inputs, cost_volume_step(True, True))
    add("flow_cost_volume-noflow", flow_inputs, cost_volume_step(False, False))
    add("flow_photometric", flow_inputs, flow_photo_step)
    add("flow_fb_check", flow_inputs, fb_check_step)
    add("smooth_grad_1st", flow_inputs, smooth1_step)
    add("flow_metrics", flow_metrics_inputs, flow_metrics_step)
    add("flow_resize", flow_metrics_inputs, flow_resize_step)
    add("range_map", splat_inputs, range_map_step)
    add("occlusion_mask", splat_inputs, occlusion_mask_step)
    add("depth_occlusion", splat_inputs, depth_occlusion_step)
    add("depth_stereo_consistency-atomic", terms_inputs(TERMS_SHAPE), dsc_step(False), {"g_src_depth": dsc_atomic()})
    add("depth_stereo_consistency-det", terms_inputs(TERMS_SHAPE), dsc_step(True))
    add("rgb_stereo_consistency", terms_inputs(TERMS_SHAPE), rsc_step(0.0))
    add("rgb_stereo_consistency-ssim", terms_inputs(PHOTO_SHAPE), rsc_step(UP.W_SSIM))
    add("depth_consistency", terms_inputs(TERMS_SHAPE), dc_step)
    add("edge_aware_smoothness", terms_inputs(TERMS_SHAPE), smooth_step)
    for op in ("ssim", "ternary"):
        for md in (1, 2):
            add("%s-md%d" % (op, md), window_inputs(md), window_step(op, md))
    big, small = DPV_SHAPES
    add("dpv_reduce", dpv_inputs(big), dpv_reduce_step)
    add("dpv_reduce-any_shape", dpv_inputs(small), dpv_reduce_step)
    add("dpv_reduce-nograd", dpv_inputs(big), dpv_reduce_nograd_step)
    add("dpv_reduce_ex-fp32", dpv_inputs(big), dpv_reduce_ex_step())
    add("dpv_reduce_ex-fp32-any_shape", dpv_inputs(small), dpv_reduce_ex_step())
    add("dpv_reduce_ex-fp16", dpv_inputs(big, torch.float16), dpv_reduce_ex_step())
    add("dpv_reduce_ex-bf16", dpv_inputs(big, torch.bfloat16), dpv_reduce_ex_step())
    add("dpv_reduce_ex-fp16-any_shape", dpv_inputs(small, torch.float16), dpv_reduce_ex_step())
    for bv_log in (True, False):
        add("dpv_expect-%s" % ("log" if bv_log else "prob"), dpv_inputs(big), dpv_expect_step(bv_log))
    add("dpv_expect-any_shape", dpv_inputs(small), dpv_expect_step(True))
    add("dpv_moments", dpv_inputs(big), dpv_moments_step)
    add("dpv_moments-any_shape", dpv_inputs(small), dpv_moments_step)
    add("dpv_fuse", dpv_inputs(big), dpv_fuse_step)
    add("dpv_fuse-any_shape", dpv_inputs(small), dpv_fuse_step)
    for form in ("label", "depth"):
        add("dpv_soft_ce-%s" % form, dpv_inputs(big), soft_ce_step(form))
    add("dpv_soft_ce-label-any_shape", dpv_inputs(small), soft_ce_step("label"))
    add("ufield", dpv_inputs(big), ufield_step)
    add("ufield-any_shape", dpv_inputs(small), ufield_step)
    add("depth_metrics", dpv_inputs(big), depth_metrics_step)
    add("depth_metrics-any_shape", dpv_inputs(small), depth_metrics_step)
    add("correlation-fp32", correlation_inputs(torch.float32), correlation_step)
    add("correlation-fp16", correlation_inputs(torch.float16), correlation_step)
    return tuple(out)


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def atomic_rules():
    """[(case name, output, Atomic)] of the table."""
    return [(c.name, n, r) for c in CASES if isinstance(c.rules, dict) for n, r in c.rules.items() if isinstance(r, Atomic)]
