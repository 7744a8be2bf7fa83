"""Golden fixture g23_ssim: the reference's SSIM (losses/loss_blocks.py:47-66) and its autograd gradients on the CPU, float32.
Build container only (imports the reference, which never travels):

    python tests/golden/make_golden_ssim.py

Inputs: tests/util_ssim.py -- for md = 1, 2, 3 on [2,3,21,37]: independent U(0,1) images; y = clamp(x + 0.05 N, 0, 1); that pair
times a random mask whose top third is 0; identical inputs; a constant image; and the one-window shape [1,3,2md+1,2md+1].
Stored: the random arrays the inputs are made of, each once (the cases of one md share x, the mask and a seeded g_out:
util_ssim.case_inputs puts a case together), and per case the reference's float32 output and x.grad, y.grad of
(SSIM(x, y, md) * g_out).sum().  Checked here: the float64 restatement of tests/util_ssim.py agrees with the reference run in
float64, and no element of a case lies within util_ssim.EDGE of a clamp edge without being on it.  Data only; nothing of the
reference is copied.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _import_reference  # noqa: E402  (also sets sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util_ssim as U  # noqa: E402


def main():
    _import_reference()
    import losses.loss_blocks as lb
    out = U.make_base()
    for name, md, kind in [(f"{kind}_md{md}", md, kind) for md in U.MDS for kind in U.KINDS]:
        x, y, g = U.case_inputs(out, kind, md)
        tx, ty = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
        dist = lb.SSIM(tx, ty, md)
        (dist * torch.from_numpy(g)).sum().backward()
        x64, y64 = torch.from_numpy(x).double(), torch.from_numpy(y).double()
        parts = U.ssim_parts(x64, y64, md)
        ref64 = lb.SSIM(x64, y64, md)
        assert (parts["raw"].clamp(0, 1) - ref64).abs().max() <= 1e-12, name
        assert not U.near_edge(parts["raw"]).any(), name
        err = float((dist.detach().double() - ref64).abs().max())
        on_edge = float(((parts["raw"] == 0) | (parts["raw"] == 1)).double().mean())
        print(f"{name}: |fp32 - fp64| = {err:.2e}, windows on a clamp edge {100 * on_edge:.0f} %, max |g_x| = {float(tx.grad.abs().max()):.2f}")
        for key, v in (("dist", dist.detach().numpy()), ("g_x", tx.grad.numpy()), ("g_y", ty.grad.numpy())):
            out[f"{name}_{key}"] = v
    path = os.path.join(HERE, "g23_ssim.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
