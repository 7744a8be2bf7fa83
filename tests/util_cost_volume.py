"""The fused cost volume of the flow network (ops.flow_cost_volume) restated from its definition, and the PWCLite fixture, for
tests/test_cost_volume_gpu.py, tests/test_pwclite_host.py, tests/test_pwclite_gpu.py, the fixture maker
(tests/golden/make_golden_pwclite.py) and tools/bench_pwclite.py.

  corr_ref           the correlation of the network's configuration, a plain padded shift-multiply-mean, in the dtype of its inputs
  cost_volume_ref    leaky_relu(corr_ref(x1, util_flow.flow_warp_ref(x2, flow, pad))); float64 = the tests' reference, float32 on the
                     CPU = their yardstick; differentiable by autograd
  inputs             the seeded inputs of a case: N(0, 1) features, N(0, 3 px) flows with util_flow's planted positions on top
  reference          per (case, pad), computed once and shared: float64 forward and gradients, the yardstick's own error against
                     them, the kept pixels of grad_flow
  check_conditions   the conditions on the inputs (not tolerances), asserted by the fixture maker on the CPU
  pwc_*              the PWCLite cases, their inputs and the fixture tests/golden/g29_pwclite.npz

Conditions on the inputs.  (a) No float64 pre-activation lies within 64 eps32 max|x1| max|warped x2| of zero (exact zeros, which
only padding produces, are exempt): the LeakyReLU kink stays out of every gradient comparison.  A pre-activation is a mean over C
products and lands that close to zero at a rate of a few in 10^4, so no seed clears a whole case; instead the x1 vector of a pixel
that breaks the condition (for either padding) is drawn again from the same N(0, 1) stream until none does -- rejection sampling
per pixel, deterministic.  (b) For grad_flow, pixels whose float64 position lies within util_flow.NEAR of an integer or of a clamp
boundary are left out; at most 1 % of the pixels that are not planted may be.
"""
import os
import types

import numpy as np
import torch
import torch.nn.functional as F

import util_flow as UF

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g29_pwclite.npz")
EPS32 = UF.EPS32
PADS = UF.PADS
SLOPE = 0.1
# ((B, C, H, W), max_displacement, with a flow): the minimum; odd sizes with partial tiles in both directions; one channel more than
# a chunk, 3 x 5 tiles; many channels on one tile; the network's coarsest level with its real channel count; md = 1; no flow
CASES = (((1, 1, 2, 2), 4, True), ((2, 3, 19, 27), 4, True), ((1, 9, 33, 70), 4, True), ((1, 67, 8, 12), 4, True),
         ((2, 192, 6, 13), 4, True), ((2, 3, 19, 27), 1, True), ((2, 3, 19, 27), 4, False), ((2, 192, 6, 13), 4, False))
KINK_MARGIN = 64     # condition (a), in eps32 max|x1| max|warped x2|
MAX_LEFT_OUT = 0.01  # condition (b)


def case_id(case):
    shape, md, with_flow = case
    return "%s_md%d_%s" % (UF.shape_key(shape), md, "flow" if with_flow else "noflow")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def corr_ref(x1, w, md):
    """[B,C,H,W] x 2 -> [B,(2 md + 1)^2,H,W]: channel (tj + md)(2 md + 1) + (ti + md) = mean_c x1[y,x] w[y+tj,x+ti], zeros outside."""
    H, W = x1.shape[2:]
    p = F.pad(w, [md] * 4)
    return torch.stack([(x1 * p[:, :, i:i + H, j:j + W]).mean(1) for i in range(2 * md + 1) for j in range(2 * md + 1)], 1)


def pre_activation_ref(x1, x2, flow, md, pad):
    return corr_ref(x1, x2 if flow is None else UF.flow_warp_ref(x2, flow, pad), md)


def cost_volume_ref(x1, x2, flow, md, pad, slope=SLOPE):
    return F.leaky_relu(pre_activation_ref(x1, x2, flow, md, pad), slope)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _near_kink(x1, x2, flow, md):
    """[B,H,W] bool: a pixel with a float64 pre-activation that breaks condition (a), for either padding."""
    bad = torch.zeros(x1.shape[0], x1.shape[2], x1.shape[3], dtype=torch.bool)
    t1, t2 = torch.from_numpy(x1).double(), torch.from_numpy(x2).double()
    for pad in (PADS if flow is not None else PADS[:1]):
        w = t2 if flow is None else UF.flow_warp_ref(t2, torch.from_numpy(flow).double(), pad)
        pre = corr_ref(t1, w, md)
        thr = KINK_MARGIN * EPS32 * float(t1.abs().max()) * float(w.abs().max())
        bad |= ((pre.abs() < thr) & (pre != 0)).any(1)
    return bad


_INPUTS = {}


def inputs(case):
    """x1, x2, flow | None, grad_out (float32 numpy) and planted [B,H,W] bool of a case (computed once).  The flow is that of
    util_flow.warp_inputs: N(0, 3 px) with the planted positions on top, at pixels spread over the batch -- exact integers, the clamp
    boundaries and one representable position either side, positions leaving the image, +-1e6."""
    if case in _INPUTS:
        return _INPUTS[case]
    (B, C, H, W), md, with_flow = case
    rs = np.random.RandomState(2900 + CASES.index(case))
    x1 = rs.randn(B, C, H, W).astype(np.float32)
    x2 = rs.randn(B, C, H, W).astype(np.float32)
    go = rs.randn(B, (2 * md + 1) ** 2, H, W).astype(np.float32)
    flow, planted = None, np.zeros((B, H, W), bool)
    if with_flow:
        flow = (3.0 * rs.randn(B, 2, H, W)).astype(np.float32)
        plants = UF._plants(H, W)
        n = min(len(plants), (B * H * W) // 2)
        for k, at in enumerate(np.linspace(0, B * H * W - 1, n).astype(int)):
            b, rem = divmod(int(at), H * W)
            y, xx = divmod(rem, W)
            planted[b, y, xx] = True
            for axis, (what, base, size) in enumerate(((plants[k][0], xx, W), (plants[k][1], y, H))):
                if what is None:
                    continue
                if what[0] == "flow":
                    flow[b, axis, y, xx] = what[1]
                else:
                    t = (base + 3 + k) % size if what[1] == "int" else what[1]
                    flow[b, axis, y, xx] = UF._aim(base, size, t, what[2])
    for _ in range(200):   # condition (a): draw the x1 vector of a pixel that breaks it again
        bad = _near_kink(x1, x2, flow, md).numpy()
        if not bad.any():
            break
        for b, y, xx in zip(*np.nonzero(bad)):
            x1[b, :, y, xx] = rs.randn(C).astype(np.float32)
    else:
        raise AssertionError("condition (a) not met: %s" % case_id(case))
    _INPUTS[case] = (x1, x2, flow, go, planted)
    return _INPUTS[case]


def check_conditions(case):
    """Asserts (a) and (b) for a case; -> (the least |pre-activation| over its threshold, the share of unplanted pixels left out)."""
    x1, x2, flow, go, planted = inputs(case)
    (B, C, H, W), md, with_flow = case
    assert not bool(_near_kink(x1, x2, flow, md).any()), case_id(case)
    t1, t2 = torch.from_numpy(x1).double(), torch.from_numpy(x2).double()
    least, share = float("inf"), 0.0
    for pad in (PADS if with_flow else PADS[:1]):
        f = torch.from_numpy(flow).double() if with_flow else None
        w = t2 if f is None else UF.flow_warp_ref(t2, f, pad)
        pre = corr_ref(t1, w, md)
        thr = KINK_MARGIN * EPS32 * float(t1.abs().max()) * float(w.abs().max())
        live = pre[pre != 0].abs()
        if live.numel():
            least = min(least, float(live.min()) / thr)
        if with_flow:
            free = ~torch.from_numpy(planted)
            if bool(free.any()):
                share = max(share, float(UF.near_jump(f, pad)[free].double().mean()))
    assert least > 1.0 and share <= MAX_LEFT_OUT, (case_id(case), least, share)
    return least, share


# ---- the reference of a case, computed once -----------------------------------------------------------------------------------------
_REFS = {}


def _run(case, pad, dtype):
    x1, x2, flow, go, _ = inputs(case)
    md = case[1]
    t = [torch.from_numpy(v).to(dtype).requires_grad_(True) for v in ((x1, x2, flow) if flow is not None else (x1, x2))]
    out = cost_volume_ref(t[0], t[1], t[2] if flow is not None else None, md, pad)
    grads = torch.autograd.grad(out, t, torch.from_numpy(go).to(dtype))
    return [out.detach()] + [g.detach() for g in grads]


def reference(case, pad):
    """-> namespace: out, g_x1, g_x2, g_flow | None (float64); err_* the float32 yardstick's own error against them (grad_flow: on
    the kept pixels); keep [B,1,H,W] bool, the pixels of grad_flow that are compared; tol_* the tolerances (util_flow.tol)."""
    key = (case, pad)
    if key in _REFS:
        return _REFS[key]
    r64, r32 = _run(case, pad, torch.float64), _run(case, pad, torch.float32)
    x1, x2, flow, go, _ = inputs(case)
    ns = types.SimpleNamespace(out=r64[0], g_x1=r64[1], g_x2=r64[2], g_flow=r64[3] if flow is not None else None, keep=None)
    # the largest value in play: the products that are summed -- x1 w for the volume, grad_out w and grad_out x1 for the gradients
    m1, m2, mg = (float(np.abs(v).max()) for v in (x1, x2, go))
    for name, a, b, scale in (("out", r64[0], r32[0], m1 * m2), ("g_x1", r64[1], r32[1], mg * m2), ("g_x2", r64[2], r32[2], mg * m1)):
        err = float((b.double() - a).abs().max())
        setattr(ns, "err_" + name, err)
        setattr(ns, "tol_" + name, UF.tol(err, scale))
    if flow is not None:
        ns.keep = ~UF.near_jump(torch.from_numpy(flow).double(), pad).unsqueeze(1).expand_as(r64[3])
        a, b = r64[3][ns.keep], r32[3].double()[ns.keep]
        ns.err_g_flow = float((b - a).abs().max()) if a.numel() else 0.0
        ns.tol_g_flow = UF.tol(ns.err_g_flow, r64[3].abs().max())
    _REFS[key] = ns
    return ns


# ---- PWCLite ------------------------------------------------------------------------------------------------------------------------
PWC_HW = (128, 192)
PWC_SEED, PWC_GAIN = 29, 0.25
# name -> (frames, reduce_dense, with_bk, B)
PWC_CASES = {"f2_reduce_bk": (2, True, True, 2), "f2_dense": (2, False, False, 1), "f3_reduce": (3, True, False, 2),
             "f5_reduce_bk": (5, True, True, 1)}
PWC_PARAMETERS = {(2, True): 2236660, (2, False): 3335434, (3, True): 2371444}
TRAIN_STEPS, TRAIN_LR = 10, 1e-4


def pwc_cfg(frames, reduce_dense):
    """(five frames run the 3-frame network on three windows: its layers are sized for n_frames = 3)"""
    return types.SimpleNamespace(upsample=True, n_frames=min(frames, 3), reduce_dense=reduce_dense)


def train_cfg():
    return types.SimpleNamespace(w_l1=0.15, w_ssim=0.85, w_ternary=0, alpha=10, warp_pad="border", occ_from_back=True, with_bk=True,
                                 w_scales=[1, 1, 1, 1, 0], w_sm_scales=[1, 0, 0, 0, 0], w_smooth=75)


def pwc_input(name):
    """x [B, 3 frames, 128, 192], float32: the 2-frame cases take the training pair; more frames are crops of one bicubically
    enlarged coarse noise image, a few pixels apart."""
    frames, _, _, B = PWC_CASES[name]
    if frames == 2:
        return train_pair()[:B].contiguous()
    H, W = PWC_HW
    g = torch.Generator().manual_seed(2930 + list(PWC_CASES).index(name))
    wide = F.interpolate(torch.randn(B, 3, 20, 28, generator=g), (H + 16, W + 16), mode="bicubic", align_corners=False)
    steps = [(8, 8), (6, 11), (5, 13), (3, 14), (2, 16)][:frames]
    return torch.cat([wide[:, :, y:y + H, x:x + W] for y, x in steps], 1).contiguous()


def train_pair():
    """The image pair of the training trajectory (and of the 2-frame cases), [2,6,128,192]: torch.randn(2,3,20,28) with generator
    seed 5, resized bicubically to 144 x 208, cropped [8:136, 8:200] and [6:134, 11:203]."""
    g = torch.Generator().manual_seed(5)
    wide = F.interpolate(torch.randn(2, 3, 20, 28, generator=g), (144, 208), mode="bicubic", align_corners=False)
    return torch.cat([wide[:, :, 8:136, 8:200], wide[:, :, 6:134, 11:203]], 1).contiguous()


def pwc_flows(res):
    """The result dict of a forward -> [(key, tensor)], every level of every list, in a fixed order ('fw.0' the finest forward flow;
    five frames: 'fw.0.0' ...)."""
    out = []
    for side in ("fw", "bw"):
        levels = res.get("flows_" + side)
        if levels is None:
            continue
        if isinstance(levels[0], (list, tuple)):
            for k, inner in enumerate(levels):
                out += [("%s.%d.%d" % (side, k, i), f) for i, f in enumerate(inner)]
        else:
            out += [("%s.%d" % (side, i), f) for i, f in enumerate(levels)]
    return out


def train_output(res):
    """flows_fw, flows_bw of a 2-frame forward -> the loss's input: per level [B,4,h,w]."""
    return [torch.cat([fw, bw], 1) for fw, bw in zip(res["flows_fw"], res["flows_bw"])]


PWC_STORE_CAP = 512


def pwc_subset(a, cap=PWC_STORE_CAP):
    """At most `cap` elements of the flattened array, evenly spread (an uneven stride: a fixed one would walk down one column)."""
    flat = np.asarray(a).reshape(-1)
    return flat[np.unique(np.linspace(0, flat.size - 1, min(cap, flat.size)).astype(np.int64))]


def pwc_tol(m, ref_err, scale):
    """m times the reference's own fp32 error of the level, with a floor of 8 eps32 scale."""
    return max(m * float(ref_err), 8 * EPS32 * float(scale))


_FIXTURE = None


def fixture():
    """tests/golden/g29_pwclite.npz as a dict, loaded once."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(GOLDEN) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE
