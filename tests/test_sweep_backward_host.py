"""Host suite of the sweep backward's per-element criterion (tests/util_sweep_backward.py: exact64_grads, pin_bound), no GPU:
the bound is one a float32 evaluation meets -- torch's CPU float32 autograd of oracle_cost stays inside it on every case small
enough to run here --; exact64_grads is the float64 oracle at other positions and nothing else; and the positions of the float32
CPU grid_sample are those of oracle.ref_cpu.sample_coords bit for bit, which is what lets one bound serve the reference's float32
evaluation and the kernel alike."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_sweep_backward as U
import test_sweep_backward_pin_gpu as P
from oracle import ref_cpu as O

# the cases of the GPU suite whose float64 blocks are small enough for the host (the others: C >= 67 at D >= 64, the soak replay)
HOST_NAMES = tuple(n for n in P.NAMES if n != "soak_778_98" and not n.startswith(("ordinary-2-67", "ordinary-4-80", "ordinary-1-67",
                                                                                   "ordinary-2-80")))


def test_the_host_cases_are_the_small_ones():
    assert len(HOST_NAMES) == len(P.NAMES) - 6 and {"ragged_3x5", "D512", "mean_6_sigma", "behind", "A", "R"} <= set(HOST_NAMES)
    for name in HOST_NAMES:
        B, V, C, H, W = P.case(name)[0]["src"].shape
        assert C * len(P.case(name)[0]["d_candi"]) * H * W <= 1 << 21, name


@pytest.mark.parametrize("metric", P.METRICS)
@pytest.mark.parametrize("name", HOST_NAMES)
def test_cpu_float32_autograd_stays_inside_the_bound(name, metric):
    """P.reference checks the float32 evaluation element by element (exactly 0 where nothing contributes) and prints the worst
    error / bound: a record, not a limit."""
    x = P.reference(name, metric, dev="cpu")
    assert bool(torch.isfinite(x["g_ref"]).all()) and bool(torch.isfinite(x["g_src"]).all())
    assert float(x["g_src"].abs().max()) > 0 and float(x["g_ref"].abs().max()) > 0
    for which in ("ref", "src"):   # what "exactly 0 where A0 == 0" rests on: A1 has nothing where A0 has nothing
        assert not bool(((x["A0_" + which] == 0) & (x["A1_" + which] != 0)).any())
    if metric == "L1":
        share = U.allowance_share(x)
        print("%s L1: the allowance touches %.4f %% of g_ref, %.4f %% of g_src" % (name, 100 * share[0], 100 * share[1]))
        assert max(share) <= 1e-2


@pytest.mark.parametrize("metric", P.METRICS)
def test_exact64_is_the_oracle_at_other_positions_only(metric):
    """Given the positions a float64 grid_sample uses (the float32 grid un-normalised in float64), exact64_grads IS float64 autograd
    of oracle_cost; with its own positions it runs the same code on sample_coords' float32 values.  The case has no sample near an
    integer (none within eight times the largest distance between the two sets of positions): the taps are the same everywhere."""
    name = "second_tile_17x33"
    b, sigma = P.case(name)
    gup = P.upstream(name)
    B, V, C, H, W = b["src"].shape
    p64, p32 = U.oracle_positions64(b), U.case_positions(b)
    for a64, a32 in zip(p64, p32):
        assert bool(torch.isfinite(a64).all())
        assert torch.equal(torch.floor(a64), torch.floor(a32.double()))
        gap = float((a32.double() - torch.round(a32.double())).abs().min())
        apart = float((a64 - a32.double()).abs().max())
        print("%s: nearest integer %.3e away, the two sets of positions at most %.3e apart" % (name, gap, apart))
        assert 0 < apart and gap > 8 * apart, (gap, apart)
    x = U.exact64_grads(b, gup, sigma, metric, positions=p64)
    r64, s64 = U.oracle_grads(b, gup, sigma, metric, torch.float64, "cpu")
    for got, want, what in ((x["g_ref"], r64, "g_ref"), (x["g_src"], s64, "g_src")):
        err, big = float((got - want).abs().max()), float(want.abs().max())
        print("%s %s %s: exact64 at float64 positions against float64 autograd: max difference %.3e of %.3e" % (name, metric, what, err, big))
        assert err <= 1e-12 * big
    y = P.reference(name, metric, dev="cpu")   # ... and at sample_coords' positions it moves by what an ulp of a position does
    for what in ("g_ref", "g_src"):
        err, big = float((y[what] - x[what]).abs().max()), float(x[what].abs().max())
        print("%s %s %s: float32 positions against float64 positions: max difference %.3e of %.3e" % (name, metric, what, err, big))
        assert err <= 1e-4 * big and (err > 0 or (metric, what) == ("L1", "g_ref"))   # (L1's g_ref has no weight in it: signs only)


def _every(b):
    """A stride over the D*HW samples of a view that keeps the per-sample images under 2^23 floats (odd: every column comes up)."""
    B, V, C, H, W = b["src"].shape
    return (len(b["d_candi"]) * (H * W) ** 2 >> 23) | 1


def _sampler_weights(b, i, v):
    """What the float32 CPU grid_sample does with every sample of view (i, v), read off its backward: the gradient of the sampled
    value with respect to a [H,W] image of its own per sample is the sample's four weights at its four taps -> [D*HW, H, W]."""
    B, V, C, H, W = b["src"].shape
    d32 = torch.from_numpy(np.asarray(b["d_candi"]).astype(np.float32))
    K = b["K"][i]
    g = O.plane_coords(K, b["R"][i, v], b["t"][i, v], b["rays"][i], d32, K.numpy()[0, 2], K.numpy()[1, 2]).reshape(-1, 1, 1, 2)[::_every(b)]
    img = torch.zeros(g.shape[0], 1, H, W, requires_grad=True)
    F.grid_sample(img, g, mode="bilinear", padding_mode="zeros", align_corners=False).sum().backward()
    return img.grad[:, 0]


def _kernel_weights(b, i, v):
    """The same image from sample_coords' positions with make_footprint's float32 arithmetic (csrc/geometry.hpp)."""
    B, V, C, H, W = b["src"].shape
    ix, iy = U.case_positions(b)
    ix, iy = ix[i, v].reshape(-1)[::_every(b)], iy[i, v].reshape(-1)[::_every(b)]
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    x, y = torch.where(fin, ix, torch.zeros_like(ix)), torch.where(fin, iy, torch.zeros_like(iy))
    xf, yf = torch.floor(x), torch.floor(y)
    w, n = x - xf, y - yf
    e, s = 1.0 - w, 1.0 - n
    x0, y0 = xf.clamp(-2, W + 1).long(), yf.clamp(-2, H + 1).long()
    out = torch.zeros(ix.numel(), H * W)
    for dx, dy, wt in ((0, 0, s * e), (1, 0, s * w), (0, 1, n * e), (1, 1, n * w)):
        xx, yy = x0 + dx, y0 + dy
        inside = fin & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).unsqueeze(1)
        out.scatter_add_(1, idx, torch.where(inside, wt, torch.zeros_like(wt)).unsqueeze(1))
    return out.reshape(-1, H, W)


@pytest.mark.parametrize("name", ("ragged_3x5", "second_tile_17x33", "sigma_minus_3", "behind"))
def test_cpu_grid_sample_has_the_positions_of_sample_coords(name):
    """Taps and float32 weights of every sample, bit for bit: the same floor, the same fraction."""
    b, _ = P.case(name)
    B, V, C, H, W = b["src"].shape
    seen = 0
    for i in range(B):
        for v in range(V):
            got, want = _sampler_weights(b, i, v), _kernel_weights(b, i, v)
            assert got.dtype == torch.float32 and want.dtype == torch.float32
            bad = int((got != want).sum())
            assert bad == 0, "%s item %d view %d: %d of %d weights differ" % (name, i, v, bad, got.numel())
            seen += int((want != 0).sum())
    print("%s: %d non-zero weights, all equal" % (name, seen))
    assert seen > 0
