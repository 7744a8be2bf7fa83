"""The kernels that share the wave layout of csrc/dpv_lanes.hpp -- dpv_reduce, dpv_reduce_ex, dpv_expect, dpv_soft_ce and the
volume form of depth_metrics -- at the shapes where a shared prologue or dispatch can go wrong: every planes-per-lane boundary
(D = 32 | 33, 64 | 65), a plane group without a plane (D = 1), the step to the any-shape kernels (D = 128 | 129), fewer quads
than a wave has lanes (4 x 8), more than one workgroup with a ragged last wave (16 x 68), H W no multiple of 4 (7 x 9), and a
volume 4 bytes off a 16-byte boundary.  What must hold bit for bit: the three expectations of a log-DPV are one tensor, the
plain reduction is the extended one without its extras, two calls give the same bits.  Each op also stays within the bound
tests/test_ops_fuzz.py has for it against float64."""
import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = 2
PLANES = (1, 4, 5, 32, 33, 64, 65, 128, 129)


def _volume(flat, shape, offset):
    """flat [n + 1] on the host -> a contiguous device volume of `shape`, on a 16-byte boundary or 4 bytes past one."""
    buf = flat.to(DEV)
    v = (buf[1:] if offset else buf[:-1]).view(shape)
    assert v.data_ptr() % 16 == (4 if offset else 0)
    return v


def _check(D, H, W, offset=False):
    tag = f"D={D} {H}x{W} offset={offset}"
    gen = torch.Generator().manual_seed(10000 * D + 100 * H + W)
    n = B * D * H * W
    x_host = torch.randn(n + 1, generator=gen) * 3.0
    x = _volume(x_host, (B, D, H, W), offset)
    dc = np.linspace(2.0, 50.0, D)
    dt = torch.tensor(dc, dtype=torch.float32).double()[None, :, None, None]
    z64 = x.cpu().double()
    lp64 = torch.log_softmax(z64, dim=1)
    mean64 = (dt * torch.softmax(z64, dim=1)).sum(1)

    # the plain reduction is the extended one without its extras; both within the fuzz test's bounds
    twice = [ops.dpv_reduce(x, dc) for _ in range(2)]
    ex_twice = [ops.dpv_reduce_ex(x, dc, want_logp=True, want_depth=True) for _ in range(2)]
    lp, dp = twice[0]
    assert torch.equal(lp, twice[1][0]) and torch.equal(dp, twice[1][1]), tag
    assert torch.equal(ex_twice[0]["logp"], ex_twice[1]["logp"]) and torch.equal(ex_twice[0]["depth"], ex_twice[1]["depth"]), tag
    assert torch.equal(lp, ex_twice[0]["logp"]), tag
    assert torch.equal(dp, ex_twice[0]["depth"]), tag
    assert (lp.cpu().double() - lp64).abs().max().item() < 3e-5 * max(1.0, float(z64.abs().max()) / 10), tag
    assert (dp.cpu().double() - mean64).abs().max().item() < 1e-4, tag

    # the three expectations of one log-DPV (the volume moved like the logits: the consumers dispatch on its address)
    logp = _volume(torch.cat([torch.zeros(1), lp.cpu().flatten()]) if offset else torch.cat([lp.cpu().flatten(), torch.zeros(1)]),
                   (B, D, H, W), offset)
    assert torch.equal(logp, lp)
    want64 = (dt * logp.cpu().double().exp()).sum(1)
    label = torch.softmax(torch.randn(B, D, H, W, generator=gen) * 2.0, dim=1).to(DEV)
    truth = (torch.rand(B, H, W, generator=gen) * 45.0 + 3.0).to(DEV)
    mask = (torch.rand(B, H, W, generator=gen) < 0.7).float().to(DEV)
    e = ops.dpv_expect(logp, dc, BV_log=True)
    assert torch.equal(e, ops.dpv_expect(logp, dc, BV_log=True)), tag
    assert (e.cpu().double() - want64).abs().max().item() < 1e-4, tag
    e_lin = ops.dpv_expect(_volume(torch.cat([logp.cpu().flatten().exp(), torch.zeros(1)]), (B, D, H, W), False), dc, BV_log=False)
    assert (e_lin.cpu().double() - want64).abs().max().item() < 1e-4, tag
    for kw in (dict(label=label), dict(depth_gt=truth, variance=0.3)):
        ce = [ops.dpv_soft_ce(logp, dc, mask=mask, want_depth=True, **kw) for _ in range(2)]
        assert torch.equal(ce[0][0], ce[1][0]) and torch.equal(ce[0][1], ce[1][1]), (tag, list(kw))
        assert torch.equal(ce[0][1], e), (tag, list(kw))
    met = [ops.depth_metrics(truth, logp=logp, d_candi=dc, mask=mask, clamp_max=dc[-1], want_depth=True) for _ in range(2)]
    assert all(torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0)) for a, b in zip(met[0], met[1])), tag
    assert torch.equal(met[0][2], e), tag


@pytest.mark.parametrize("size", [(4, 8), (16, 68), (7, 9)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("D", PLANES)
def test_shared_layout_kernels_agree_bit_for_bit(D, size):
    _check(D, *size)


@pytest.mark.parametrize("D", (5, 64))
def test_volume_four_bytes_off_alignment(D):
    _check(D, 16, 68, offset=True)
