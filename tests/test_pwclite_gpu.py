"""GPU suite: models.pwclite.PWCLite on the device against the fixture of the reference's run (tests/golden/g29_pwclite.npz).

  flows      every case, with fused_cost off and on, every level against float64.  The yardstick is the reference's own fp32 error
             of the level (fixture); the tolerance is M times it, with a floor of 8 eps32 max |flow|.  M: DESIGN.md section 6.12 --
             it starts at the project's 2 and is raised, by powers of two, only as far as the UNFUSED path needs (PyTorch's device
             convolutions round differently from the CPU's, and that path holds nothing else but ops merged and pinned earlier);
             the fused path must meet the same M and M is never fitted to it.
  training   ten Adam steps under this package's unFlowLoss with fused_cost: finite, last / first <= 1 - 0.5 (1 - r) with r the
             reference's recorded ratio, step 0's four values within the M-rule of the fixture's
  launches   forward_2_frames at 128 x 192 launches the fused forward kernel exactly 5 times and neither the flow_warp forward kernel
             nor a correlation forward kernel
Every test prints the figures it asserts on.
"""
import numpy as np
import pytest
import torch

import util_cost_volume as U
from pdepth_amd import synth
from pdepth_amd.losses.flow_loss import unFlowLoss
from pdepth_amd.models.pwclite import PWCLite

pytestmark = pytest.mark.gpu

M = 4   # the unfused path reached 1.29 times the tolerance of M = 2 (one level of one case); it meets 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _model(frames, reduce_dense, fused, dev):
    model = PWCLite(U.pwc_cfg(frames, reduce_dense), fused_cost=fused)
    synth.seed_weights(model, seed=U.PWC_SEED, gain=U.PWC_GAIN)
    return model.to(dev)


@pytest.mark.parametrize("fused", (False, True), ids=("composed", "fused"))
@pytest.mark.parametrize("name", list(U.PWC_CASES))
def test_flows_against_float64(name, fused, dev):
    frames, reduce_dense, with_bk, _ = U.PWC_CASES[name]
    fx = U.fixture()
    model = _model(frames, reduce_dense, fused, dev)
    with torch.no_grad():
        flows = U.pwc_flows(model(U.pwc_input(name).to(dev), with_bk=with_bk))
    assert len(flows) == len([k for k in fx if k.startswith(name + ".") and k.endswith(".v64")])
    worst, failed = 0.0, []
    for key, f in flows:
        ref, ref_err, scale = fx[f"{name}.{key}.v64"], float(fx[f"{name}.{key}.err"]), float(fx[f"{name}.{key}.max"])
        err = float(np.abs(U.pwc_subset(f.double().cpu().numpy()) - ref).max())
        tol = U.pwc_tol(M, ref_err, scale)
        worst = max(worst, err / tol)
        print(f"{name} fused={fused} {key}: |flow - float64| {err:.2e}, reference's fp32 error {ref_err:.2e}, max |flow| {scale:.2f}, "
              f"tolerance {tol:.2e}, error / reference's {err / ref_err:.2f}")
        if err > tol:
            failed.append((key, err, tol))
    print(f"{name} fused={fused}: worst error / tolerance {worst:.2f} at M = {M}")
    assert not failed, failed


def test_training_trajectory(dev):
    fx = U.fixture()
    ref_totals, s32, s64 = fx["train.totals32"], fx["train.step0_32"], fx["train.step0_64"]
    model = _model(2, True, True, dev)
    loss_fn = unFlowLoss(U.train_cfg())
    opt = torch.optim.Adam(model.parameters(), lr=U.TRAIN_LR)
    target = U.train_pair().to(dev)
    rows = []
    for _ in range(U.TRAIN_STEPS):
        opt.zero_grad()
        vals = loss_fn(U.train_output(model(target, with_bk=True)), target)
        vals[0].backward()
        opt.step()
        rows.append(torch.stack([v.detach() for v in vals]))
    rows = torch.stack(rows).double().cpu().numpy()
    r = float(ref_totals[-1] / ref_totals[0])
    bound = 1 - 0.5 * (1 - r)
    ratio = float(rows[-1, 0] / rows[0, 0])
    print("totals:", " ".join(f"{v:.4f}" for v in rows[:, 0]), f"; last / first {ratio:.3f}, the reference's {r:.3f}, bound {bound:.3f}")
    assert np.isfinite(rows).all()
    assert ratio <= bound
    # step 0: the four values against float64; the yardstick is the reference's own fp32 error of them (the largest of the four:
    # they are sums of one another), the scale the largest value
    tol = U.pwc_tol(M, float(np.abs(s32 - s64).max()), float(np.abs(s64).max()))
    err = np.abs(rows[0] - s64)
    print(f"step 0: {rows[0]} against {s64}: errors {err}, tolerance {tol:.2e} (M = {M})")
    assert float(err.max()) <= tol


def test_launch_count(dev):
    from torch.profiler import ProfilerActivity, profile
    model = _model(2, True, True, dev)
    x = U.train_pair().to(dev)
    with torch.no_grad():
        pyramids = [model.feature_pyramid_extractor(x[:, 3 * i:3 * i + 3]) + [x[:, 3 * i:3 * i + 3]] for i in range(2)]
        model.forward_2_frames(*pyramids)   # (warm-up: lazy initialisation stays out of the trace)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            model.forward_2_frames(*pyramids)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    fused = [n for n in names if "flow_cost_volume_kernel" in n]
    warp = [n for n in names if "flow_warp_kernel" in n]
    corr = [n for n in names if "correlation_fwd" in n or "correlation_general" in n]
    print(f"{len(names)} device events: {len(fused)} fused cost volumes, {len(warp)} flow_warp, {len(corr)} correlation")
    assert len(names) > 5, "the profiler recorded no device kernels"
    assert len(fused) == 5 and not warp and not corr
