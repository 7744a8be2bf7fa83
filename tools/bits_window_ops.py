"""The bits of every op built on csrc/window_tile.hpp and csrc/loss_terms_sum.hpp: a refactor of those files leaves every digest as
it was.  Run it once with PDEPTH_LIB naming the library to compare with and once without, each in a fresh process:

    PDEPTH_LIB=/path/to/other/libpdepth_hip.so python tools/bits_window_ops.py
    python tools/bits_window_ops.py

Each prints ONE JSON line, {case: SHA-256 of the output's bytes}, of ssim, ternary, loss_photo, flow_photo and loss_rsc / dsc / dc /
smooth / smooth1, forward and backward, on seeded inputs made on the CPU: at the least size (one window, a tile that is all halo), at
[2,3,17,130] (two or three tile rows, three tile columns, ragged both ways) and at one workload shape per fused op.  It gates nothing."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdepth_amd  # noqa: E402,F401
from pdepth_amd import _native as N  # noqa: E402

DEV, GEN, OUT = torch.device("cuda:0"), torch.Generator(device="cpu").manual_seed(1234), {}


def rand(*shape):
    return torch.rand(*shape, generator=GEN).to(DEV)


def put(case, *tensors):
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    OUT.update({f"{case}/{i}": sha(t) for i, t in enumerate(tensors) if t is not None})


def camera(B, H, W):
    """Kinv [B,3,3], proj [B,3,4], the pose's third row [1,4], K [B,3,3] of a 0.54 m stereo baseline."""
    K = torch.tensor([[0.85 * W, 0.0, 0.5 * W], [0.0, 1.1 * H, 0.49 * H], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    pose = torch.tensor([[1.0, 0.0, 0.0, -0.54], [0.0, 1.0, 0.0, 0.01], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    return (torch.linalg.inv(K).contiguous().to(DEV), torch.matmul(K, pose[None, :3, :]).contiguous().to(DEV),
            pose[2:3].contiguous().to(DEV), K.to(DEV))


def window_ops(shape, md):
    B, C, H, W = shape
    x, y, tag = rand(*shape), rand(*shape), f"{list(shape)}/md{md}"
    put(f"ssim/{tag}", N.ssim(x, y, md), *N.ssim_backward(x, y, rand(B, C, H - 2 * md, W - 2 * md) - 0.5, md))
    put(f"ternary/{tag}", N.ternary(x, y, md), *N.ternary_backward(x, y, rand(B, 1, H, W) - 0.5, md))


def photo(shape, md, w):
    B, _, H, W = shape
    src, tgt, depth = rand(*shape), rand(*shape), 8.0 + 28.0 * rand(B, H, W)
    Kinv, proj = camera(B, H, W)[:2]
    value, count = N.loss_photo(src, tgt, depth, Kinv, proj, w, md)
    put(f"loss_photo/{list(shape)}/md{md}/w{w}", value, count,
        N.loss_photo_backward(src, tgt, depth, Kinv, proj, count, 1.0 + rand(B), w, md))


def flow_photo(shape, pad, weights):
    B, _, H, W = shape
    im, other, flow, mask = rand(*shape), rand(*shape), 6.0 * rand(B, 2, H, W) - 3.0, (rand(B, 1, H, W) > 0.2).float()
    value, count = N.flow_photo(im, other, flow, mask, *weights, pad=pad)
    put(f"flow_photo/{list(shape)}/{pad}/{weights}", value, count,
        N.flow_photo_backward(im, other, flow, mask, count, 1.0 + rand(1), *weights, pad=pad))


def pixel_terms(B, H, W):
    rgb, rgb2, depth, depth2 = rand(B, 3, H, W), rand(B, 3, H, W), 8.0 + 28.0 * rand(B, H, W), 8.0 + 28.0 * rand(B, H, W)
    (Kinv, proj, pose_row, K), g = camera(B, H, W), 1.0 + rand(B)
    value, count = N.loss_rsc(rgb, rgb2, depth, Kinv, proj)
    put("loss_rsc", value, count, N.loss_rsc_backward(rgb, rgb2, depth, Kinv, proj, count, g))
    dsc = (depth2, depth, (rand(B, H, W) > 0.2).float(), Kinv, proj, pose_row, K)
    value, count = N.loss_dsc(*dsc)
    put("loss_dsc", value, count, *N.loss_dsc_backward(*dsc, count, g, want_src=False))   # (g_src is a sum of atomics)
    small = 8.0 + 28.0 * rand(B, H // 4, W // 4)
    value, count = N.loss_dc(depth, small)
    put("loss_dc", value, count, *N.loss_dc_backward(depth, small, count, g))
    put("loss_smooth", N.loss_smooth(depth, rgb), N.loss_smooth_backward(depth, rgb, g))
    flo = 6.0 * rand(B, 2, H, W) - 3.0
    put("loss_smooth1", N.loss_smooth1(flo, rgb, 10.0), N.loss_smooth1_backward(flo, rgb, 10.0, 1.0 + rand(1)))


def main():
    with torch.no_grad():
        for md in (1, 2, 3):
            window_ops((1, 3, 2 * md + 1, 2 * md + 1), md)
            window_ops((2, 3, 17, 130), md)
            for w in (0.85, 0.0):
                photo((2, 3, 17, 130), md, w)
        for shape in ((1, 3, 3, 3), (2, 3, 17, 130)):
            for pad in ("border", "zeros"):
                for weights in ((0.15, 0.85, 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
                    flow_photo(shape, pad, weights)
        pixel_terms(2, 17, 130)
        flow_photo((4, 3, 256, 832), "border", (0.15, 0.85, 0.5))
        photo((4, 3, 256, 512), 1, 0.85)
    print(json.dumps(OUT))


if __name__ == "__main__":
    main()
