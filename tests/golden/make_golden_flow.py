"""Golden fixture g28_flow: the reference's flow_warp with torch autograd's gradients, its smooth_grad_1st and its unFlowLoss
(utils/warp_utils.py, losses/loss_blocks.py, losses/flow_loss.py) on the CPU.  Build container only (imports the reference, which
never travels):

    python tests/golden/make_golden_flow.py

Inputs: tests/util_flow.py.  Stored per warp case (util_flow.SHAPES): the flow with its planted positions and the mask of planted
pixels by value; x and grad_out are the seeded draws of util_flow.warp_inputs (numpy's legacy generator, a fixed stream) and are
not stored -- C = 192 alone would be the size of the whole fixture.  Per padding: out, grad_x, grad_flow.  smooth: flo, image,
value, gradient.  Per unFlowLoss case (util_flow.UNFLOW_CASES; the pyramid and the image pair once, by value): the four values and
the gradient with respect to every level.

Every reference output is kept twice, from the reference run in float32 (`<key>32`) and in float64 (`<key>64d`: the float64 result
minus the float32 one, as float32 -- util_flow.ref64 adds them back, exact to 1e-7 of the difference), and a large array as every
k-th element (util_flow.subset, at most STORE_CAP elements): the fixture stays small.  The float32 gradients of the unFlowLoss
cases are kept whole: the GPU tests take the reference's own fp32 error from them, and a maximum over a subset of the elements
would understate it (measured: by up to 40 times at the finest level).

Checked here: the float64 restatements of tests/util_flow.py agree with the reference's float64 run to 1e-10 of the largest value
(forward-backward masks and occlusion masks: every pixel); the masks of the unFlowLoss inputs keep a margin of 3e-4 (range map
against its threshold, the check's |lhs - rhs|), in float64 and for the float32 run, and none of their sample positions lies
within util_flow.NEAR of an integer or of a clamp boundary -- conditions on the inputs, not tolerances: a seed that breaks them is
changed (util_flow.UNFLOW_SEED).  Data only; nothing of the reference is copied.
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util_flow as U  # noqa: E402


def _close(mine, ref, what):
    scale = max(1.0, float(ref.abs().max()))
    err = float((mine - ref).abs().max())
    assert err <= 1e-10 * scale, (what, err, scale)


def _keep(out, key, v32, v64, whole=False):
    """whole: the float32 result in full -- the GPU tests take the reference's own fp32 error from it, over every element."""
    v32, v64 = v32.detach(), v64.detach()
    out[key + "32"] = v32.numpy() if whole else U.subset(v32.numpy())
    out[key + "64d"] = U.subset((v64 - v32.double()).float().numpy())


def _warp_case(wu, shape, out):
    name = "warp_" + U.shape_key(shape)
    x, flow, go, planted = U.warp_inputs(shape)
    out[name + ".flow"], out[name + ".planted"] = flow, planted.astype(np.uint8)
    for pad in U.PADS:
        res = {}
        for dtype in (torch.float32, torch.float64):
            tx, tf = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(flow).to(dtype).requires_grad_(True)
            o = wu.flow_warp(tx, tf, pad=pad)
            gx, gf = torch.autograd.grad(o, (tx, tf), torch.from_numpy(go).to(dtype))
            res[dtype] = (o, gx, gf)
        tx, tf = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(flow).double().requires_grad_(True)
        o = U.flow_warp_ref(tx, tf, pad)
        gx, gf = torch.autograd.grad(o, (tx, tf), torch.from_numpy(go).double())
        _close(o, res[torch.float64][0], (name, pad, "out"))
        _close(gx, res[torch.float64][1], (name, pad, "grad_x"))
        keep = ~U.near_jump(tf.detach(), pad).unsqueeze(1).expand_as(gf)
        _close(gf[keep], res[torch.float64][2][keep], (name, pad, "grad_flow"))
        free = ~torch.from_numpy(planted)
        share = float(U.near_jump(tf.detach(), pad)[free].double().mean()) if bool(free.any()) else 0.0
        for key, i in (("out", 0), ("grad_x", 1), ("grad_flow", 2)):
            _keep(out, f"{name}.{pad}.{key}", res[torch.float32][i], res[torch.float64][i])
        e = [float((res[torch.float32][i].double() - res[torch.float64][i]).abs().max()) for i in range(2)]
        print(f"{name} {pad}: fp32 error out {e[0]:.1e}, grad_x {e[1]:.1e}; left out of grad_flow (not planted) {100 * share:.2f} %")


def main():
    _import_reference()
    import utils.warp_utils as wu
    import losses.loss_blocks as lb
    import losses.flow_loss as fl
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for shape in U.SHAPES:
            _warp_case(wu, shape, out)

        for shape in U.FB_SHAPES:   # (nothing stored: the restatement's masks are the reference's, every pixel, both precisions)
            f12, f21 = (torch.from_numpy(v) for v in U.fb_inputs(shape))
            occ64, m64 = U.fb_check_ref(f12.double(), f21.double())
            assert torch.equal(occ64, wu.get_occu_mask_bidirection(f12.double(), f21.double()).float()), shape
            flips = int((wu.get_occu_mask_bidirection(f12, f21) != occ64).sum())
            print(f"fb {shape}: occluded {float(occ64.mean()):.2f}, least margin {float(m64.min()):.1e}, "
                  f"within 1e-4: {int((m64 < 1e-4).sum())}, fp32 flips {flips}")

        flo, image, alpha = U.smooth_inputs()
        out["smooth.flo"], out["smooth.image"], out["smooth.alpha"] = flo, image, np.float64(alpha)
        res = {}
        for dtype in (torch.float32, torch.float64):
            tf, ti = torch.from_numpy(flo).to(dtype).requires_grad_(True), torch.from_numpy(image).to(dtype)
            v = lb.smooth_grad_1st(tf, ti, alpha)
            res[dtype] = (v, torch.autograd.grad(v, tf)[0])
        tf = torch.from_numpy(flo).double().requires_grad_(True)
        v = U.smooth_ref(tf, torch.from_numpy(image).double(), alpha)
        _close(v, res[torch.float64][0], "smooth value")
        _close(torch.autograd.grad(v, tf)[0], res[torch.float64][1], "smooth grad")
        _keep(out, "smooth.value", res[torch.float32][0].reshape(1), res[torch.float64][0].reshape(1))
        _keep(out, "smooth.grad", res[torch.float32][1], res[torch.float64][1])

        flows, target = U.unflow_inputs()
        for i, f in enumerate(flows):
            out[f"unflow.flow{i}"] = f
        out["unflow.target"] = target
        for f in flows:   # no sample position near a jump of d out / d flow, either direction, either padding
            for part in (f[:, :2], f[:, 2:]):
                for pad in U.PADS:
                    assert not bool(U.near_jump(torch.from_numpy(part).double(), pad).any()), "a position near a jump: change UNFLOW_SEED"
        for case in U.UNFLOW_CASES:
            name, cfg = U.unflow_name(*case), U.unflow_cfg(*case)
            res = {}
            for dtype in (torch.float32, torch.float64):
                tfl = [torch.from_numpy(f).to(dtype).requires_grad_(True) for f in flows]
                with contextlib.redirect_stdout(io.StringIO()):
                    vals = fl.unFlowLoss(cfg)(tfl, torch.from_numpy(target).to(dtype))
                res[dtype] = (torch.stack([v.detach() for v in vals]), torch.autograd.grad(vals[0], tfl))
                _, margin = U.unflow_ref(cfg, [t.detach() for t in tfl], torch.from_numpy(target).to(dtype))
                assert margin > 3e-4, (name, dtype, margin, "a mask pixel near its threshold: change UNFLOW_SEED")
            tfl = [torch.from_numpy(f).double().requires_grad_(True) for f in flows]
            vals, margin = U.unflow_ref(cfg, tfl, torch.from_numpy(target).double())
            _close(torch.stack([v.detach() for v in vals]), res[torch.float64][0], (name, "values"))
            for i, g in enumerate(torch.autograd.grad(vals[0], tfl)):
                _close(g, res[torch.float64][1][i], (name, "grad", i))
            _keep(out, f"{name}.values", res[torch.float32][0], res[torch.float64][0])
            for i in range(len(flows)):
                _keep(out, f"{name}.grad{i}", res[torch.float32][1][i], res[torch.float64][1][i], whole=True)
            e = float((res[torch.float32][0].double() - res[torch.float64][0]).abs().max())
            print(f"{name}: total {float(vals[0]):.6f} warp {float(vals[1]):.6f} smooth {float(vals[2]):.6f}, mask margin {margin:.1e}, "
                  f"fp32 error of the values {e:.1e}")
    path = os.path.join(HERE, "g28_flow.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
