"""The bits of the ops whose kernels live in csrc/dpv_fuse.hip, csrc/dpv_moments.hip, csrc/correlation.hip, csrc/inverse_warp.hip and
of the gather of the fused cost volume's backward (csrc/cost_volume.hip): moving or restating that code leaves every digest as it
was.  Run it once with PDEPTH_LIB naming the library to compare with and once without, each in a fresh process:

    PDEPTH_LIB=/path/to/other/libpdepth_hip.so python tools/bits_moved_ops.py
    python tools/bits_moved_ops.py

Each prints ONE JSON line, {case: SHA-256 of the output's bytes}, on seeded inputs made on the CPU:
  dpv_fuse (fused and log) and dpv_moments (both bv_log) at [2,D,5,70], D = 5, 64, 100, 130: both register forms and the re-reading
      form, a ragged last block
  correlation forward and backward (both gradients, each alone) at [2,9,17,35]: (md, stride2) = (1,1), (4,1), (4,2) and a
      configuration of the general kernels (stride1 2)
  flow_cost_volume forward and its deterministic backward, with and without a flow, at [1,1,2,2] and [2,9,17,35], md 1 and 4
  inverse_warp in both modes and the point gradient of its backward at [2,3,9,37] (the image gradient is a sum of float atomics)
  the two gathers at one workload shape, [4,64,48,104], md 4
It gates nothing."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import _native as N  # noqa: E402

DEV, GEN, OUT = torch.device("cuda:0"), torch.Generator(device="cpu").manual_seed(4321), {}
SLOPE = 0.1


def rand(*shape):
    return torch.rand(*shape, generator=GEN).to(DEV)


def randn(*shape):
    return torch.randn(*shape, generator=GEN).to(DEV)


def put(case, *tensors):
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    OUT.update({f"{case}/{i}": sha(t) for i, t in enumerate(tensors) if t is not None})


def dpv(D):
    B, H, W = 2, 5, 70
    logp = torch.log_softmax(randn(B, D, H, W), dim=1)
    dc = torch.linspace(5.0, 40.0, D).to(DEV)
    mask = (rand(B, H, W) > 0.6).float()
    dmap = (6.0 + 30.0 * rand(B, H, W)) * mask
    put(f"dpv_fuse/D{D}", *N.dpv_fuse(logp, dmap, mask, dc, 0.3, 1e-5))
    put(f"dpv_moments/D{D}/log", *N.dpv_moments(logp, dc, bv_log=True))
    put(f"dpv_moments/D{D}/plain", *N.dpv_moments(logp.exp(), dc, bv_log=False))


def correlation(shape, cfg):
    """cfg = (pad, kernel, max_displacement, stride1, stride2)"""
    x1, x2 = randn(*shape), randn(*shape)
    out = N.correlation_forward(x1, x2, *cfg)
    go = randn(*out.shape)
    tag = f"correlation/{list(shape)}/{cfg}"
    put(tag + "/forward", out)
    put(tag + "/backward", *N.correlation_backward(x1, x2, go, *cfg))
    put(tag + "/backward_x1", *N.correlation_backward(x1, x2, go, *cfg, want2=False))
    put(tag + "/backward_x2", *N.correlation_backward(x1, x2, go, *cfg, want1=False))


def cost_volume(shape, md, with_flow):
    B, _, H, W = shape
    x1, x2 = randn(*shape), randn(*shape)
    flow = 3.0 * randn(B, 2, H, W) if with_flow else None
    out = N.flow_cost_volume(x1, x2, flow, md, SLOPE)
    go = randn(*out.shape)
    tag = f"flow_cost_volume/{list(shape)}/md{md}/{'flow' if with_flow else 'noflow'}"
    put(tag + "/forward", out)
    put(tag + "/backward", *N.flow_cost_volume_backward(x1, x2, flow, out, go, md, SLOPE, deterministic=True))
    put(tag + "/backward_x1", *N.flow_cost_volume_backward(x1, x2, flow, out, go, md, SLOPE, want_x2=False, want_flow=False, deterministic=True))
    put(tag + "/backward_x2", *N.flow_cost_volume_backward(x1, x2, flow, out, go, md, SLOPE, want_x1=False, want_flow=False, deterministic=True))


def inverse_warp(B, C, H, W):
    K = torch.tensor([[0.85 * W, 0.0, 0.5 * W], [0.0, 1.1 * H, 0.49 * H], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    pose = torch.tensor([[1.0, 0.0, 0.0, -0.54], [0.0, 1.0, 0.0, 0.01], [0.0, 0.0, 1.0, 0.0]])
    Kinv, proj = torch.linalg.inv(K).contiguous().to(DEV), torch.matmul(K, pose[None]).contiguous().to(DEV)
    img, depth, go = rand(B, C, H, W), 8.0 + 28.0 * rand(B, H, W), randn(B, C, H, W)
    for mode in ("bilinear", "nearest"):
        out, valid = N.inverse_warp(img, depth, Kinv, proj, mode)
        put(f"inverse_warp/{mode}", out, valid.to(torch.uint8))
        put(f"inverse_warp_backward/{mode}", *N.inverse_warp_backward(img, depth, Kinv, proj, go, mode, want_img=False))


def main():
    with torch.no_grad():
        for D in (5, 64, 100, 130):
            dpv(D)
        for cfg in ((1, 1, 1, 1, 1), (4, 1, 4, 1, 1), (4, 1, 4, 1, 2), (4, 1, 4, 2, 1)):
            correlation((2, 9, 17, 35), cfg)
        for shape in ((1, 1, 2, 2), (2, 9, 17, 35)):
            for md in (1, 4):
                for with_flow in (False, True):
                    cost_volume(shape, md, with_flow)
        inverse_warp(2, 3, 9, 37)
        correlation((4, 64, 48, 104), (4, 1, 4, 1, 1))
        cost_volume((4, 64, 48, 104), 4, False)
        cost_volume((4, 64, 48, 104), 4, True)
    print(json.dumps(OUT))


if __name__ == "__main__":
    main()
