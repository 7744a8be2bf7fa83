"""Golden fixture g26_ternary: the reference's TernaryLoss (losses/loss_blocks.py:8-44) and its autograd gradients on the CPU,
float32.  Build container only (imports the reference, which never travels):

    python tests/golden/make_golden_ternary.py

Inputs: tests/util_ternary.py -- for md = 1, 2, 3 on [2,3,21,37]: independent U(0,1) images; y = clamp(x + 0.05 N, 0, 1); that pair
times a random mask whose top third is 0; identical inputs; a constant image; and the one-interior-pixel shape [1,3,2md+1,2md+1].
Stored: the random arrays the inputs are made of, each once (the cases share x, the second images, the mask and a seeded g_out:
util_ternary.case_inputs puts a case together), and per case the reference's float32 output and im.grad, im_warp.grad of
(TernaryLoss(im, im_warp, md) * g_out).sum().  Checked here: the float64 restatement of tests/util_ternary.py agrees with the
reference run in float64 to 1e-12, output and gradients (the gradients relative to their largest element), and the identical and
constant cases are exactly 0 in the reference's float32, gradients included.  Data only; nothing of the reference is copied.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util_ternary as U  # noqa: E402


def _run(fn, x, y, g, md, dtype):
    tx, ty = torch.from_numpy(x).to(dtype).requires_grad_(True), torch.from_numpy(y).to(dtype).requires_grad_(True)
    dist = fn(tx, ty, md)
    (dist * torch.from_numpy(g).to(dtype)).sum().backward()
    return dist.detach(), tx.grad, ty.grad


def main():
    _import_reference()
    import losses.loss_blocks as lb
    out = U.make_base()
    for name, md, kind in [(f"{kind}_md{md}", md, kind) for md in U.MDS for kind in U.KINDS]:
        x, y, g = U.case_inputs(out, kind, md)
        dist, gx, gy = _run(lb.TernaryLoss, x, y, g, md, torch.float32)
        ref64 = _run(lb.TernaryLoss, x, y, g, md, torch.float64)
        mine64 = _run(U.ternary_dist, x, y, g, md, torch.float64)
        assert (mine64[0] - ref64[0]).abs().max() <= 1e-12, name
        for a, b in zip(mine64[1:], ref64[1:]):
            assert (a - b).abs().max() <= 1e-12 * max(1.0, float(b.abs().max())), name
        if kind in ("same", "const"):
            assert not dist.any() and not gx.any() and not gy.any(), name
        err = [float((a.double() - b).abs().max()) for a, b in zip((dist, gx, gy), ref64)]
        print(f"{name}: |fp32 - fp64| = {err[0]:.2e}; g_x {err[1]:.2e}, g_y {err[2]:.2e} against max |g| = "
              f"{float(ref64[1].abs().max()):.2f}, {float(ref64[2].abs().max()):.2f}")
        for key, v in (("dist", dist.numpy()), ("g_x", gx.numpy()), ("g_y", gy.numpy())):
            out[f"{name}_{key}"] = v
    path = os.path.join(HERE, "g26_ternary.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
