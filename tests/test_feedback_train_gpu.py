"""GPU suite: BaseModel, nmode default_feedback, trains -- the last op on that path without a backward, warp_feature, now has one
(csrc/warp_bwd.hip, reached through ops.warp_feature(differentiable=True)).  Two chained frames at B = 1, V = 1, D = 64 on a
256 x 256 image (a 64 x 64 sweep: the smallest the encoder's pyramid accepts); the second frame's prev_output is the first one's
refined log-DPV, detached and reduced to a quarter, as the reference's training loop feeds it back
(trainer/default_trainer.py:144-146).  The twin runs the same weights with warp_feature replaced by a torch composite
(oracle plane_coords + F.grid_sample on [D,1,H,W]) under autograd; the other HIP ops stay, their backwards are pinned elsewhere
(tests/test_sweep_backward.py, tests/test_fuse_backward.py).

Conditioning of the comparison, measured on an MI355X on exactly these inputs (relative difference of a base_encoder
parameter's gradient, worst parameter):
  * the training step against ITSELF, nothing patched, two deep copies: 4.6e-3 (152 of 181 parameters above 1e-3); the twin
    against itself 3.3e-3.  The backward of the convolutions is not reproducible by default, and the gradient arriving at the
    warp already differs by 1.4e-3 between two runs.  With torch.backends.cudnn.deterministic and sweep_deterministic the step
    repeats bit for bit (0 on every parameter), the twin to 2e-5 (grid_sample's own atomics).  So every step here runs with both
    set -- the scope of tests/test_det_scatter_gpu.py: the convolutions are PyTorch's / MIOpen's to make reproducible.
  * the composite's forward is not the kernel's: its positions come from device matmuls and grid_sample's own un-normalisation,
    and its output differs from the kernel's by 1e-6 (relative, in norm; the kernel is the one pinned to float64 in
    test_warps_gpu.py).  The network behind the warp turns that into 2.7e-3 of the gradient that ARRIVES at the warp, flags on,
    before either backward of the warp has run, and into up to 4e-3 on 179 of 181 parameters.  A gradient comparison has to be
    made at one point: the twin therefore returns the kernel's forward values and the composite's gradient
    (composite + (kernel - composite).detach()).  What then differs is the warp's backward alone, which is what the comparison
    is for: 2.3e-5 on the worst parameter, the twin's own run-to-run figure.  The tolerance is the project's 1e-3 either way."""
import copy

import pytest
import torch
import torch.nn.functional as F

import pdepth_amd  # noqa: F401
from pdepth_amd import ops, synth
from pdepth_amd.losses.get_loss import get_loss
from pdepth_amd.models.get_model import get_model
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

B, H, W, D = 1, 256, 256, 64
TWIN_TOL = 1e-3   # the project's twin tolerance (tests/test_fuse_backward.py::test_upsample_model_trains)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _torch_warp_feature(src, K, R, t, rays, cxcy, d_candi, blas=None, differentiable=False, deterministic=None):
    """The torch composite: channel k of every view through F.grid_sample with the grid of plane k."""
    Bn, V, Dn, h, w = src.shape
    dc = ops.d_candi_tensor(d_candi, src.device)
    out = []
    for i in range(Bn):
        views = []
        for v in range(V):
            grid = O.plane_coords(K[i], R[i, v], t[i, v], rays[i], dc, cxcy[i, 0], cxcy[i, 1]).reshape(Dn, h, w, 2)
            views.append(F.grid_sample(src[i, v].unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0])
        out.append(torch.stack(views))
    return torch.stack(out)


def _twin_warp_feature(src, *args, blas=None, differentiable=False, deterministic=None):
    """The composite's gradient at the kernel's forward values (module docstring)."""
    comp = _torch_warp_feature(src, *args)
    with torch.no_grad():
        value = _KERNEL_WARP(src, *args, blas=blas)
    return comp + (value - comp).detach()


_KERNEL_WARP = ops.warp_feature


class _reproducible_convs:
    """torch.backends.cudnn.deterministic for the steps of this file: this test is the caller whose business that is."""

    def __enter__(self):
        self.was = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = self.was
        return False


def _step(model, frames, targets):
    """One two-frame training step, reproducibly: -> loss (backward done)."""
    model.sweep_deterministic = True
    with _reproducible_convs():
        loss = _two_frame_loss(model, frames, targets)
        loss.backward()
    return float(loss.detach())


def _model(dev, cfg=None):
    torch.manual_seed(0)
    model = get_model(cfg or synth.default_cfg("default_feedback"), 0)
    synth.seed_weights(model, seed=31)
    return model.to(dev).train()


def _frames(dev):
    return [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v)
             for k, v in synth.make_model_input(seed, B=B, V=1, H=H, W=W, D=D, pose="mono").items()} for seed in (3100, 3101)]


def _targets(dev):
    gen = torch.Generator().manual_seed(2)
    return [(torch.rand(B, H, W, generator=gen) * 30 + 5).to(dev) for _ in range(2)]


def _depth_l1(bv, d_candi, target):
    depth = ops.dpv_expect(bv, d_candi, BV_log=True)
    tgt = F.interpolate(target.unsqueeze(1), size=depth.shape[-2:], mode="nearest").squeeze(1)
    return (depth - tgt).abs().mean()


def _two_frame_loss(model, frames, targets):
    """The depth-L1 loss of tests/test_fuse_backward.py::_model_loss on output[-1] (BV_upd) and output_refined[-1] of two chained
    frames; prev_output is detached by the loop, as in the reference's."""
    prev, loss = None, 0
    for inp, target in zip(frames, targets):
        inp = dict(inp, prev_output=prev)
        out = model([inp])[0]
        for bv in (out["output"][-1], out["output_refined"][-1]):
            loss = loss + _depth_l1(bv, inp["d_candi"], target)
        prev = F.interpolate(out["output_refined"][-1].detach(), scale_factor=0.25, mode="nearest")
    return loss


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def trained(dev):
    """(pristine copy of the model, frames, targets, loss, gradients) of one two-frame step through the HIP backward; computed once."""
    model = _model(dev)
    pristine = copy.deepcopy(model)
    frames, targets = _frames(dev), _targets(dev)
    loss = _step(model, frames, targets)
    return pristine, frames, targets, loss, _grads(model)


def test_feedback_model_matches_its_torch_twin(dev, trained, monkeypatch):
    pristine, frames, targets, loss, grads = trained
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads.values())
    twin = copy.deepcopy(pristine)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "warp_feature", _twin_warp_feature)
        tloss = _step(twin, frames, targets)
    print("default_feedback: loss", loss, "twin", tloss)
    assert abs(loss - tloss) <= TWIN_TOL * abs(tloss)
    checked, worst = 0, 0.0
    for n, p in twin.named_parameters():
        if not n.startswith("base_encoder") or p.grad is None:
            continue
        den = float(p.grad.norm())
        if den == 0:
            continue
        rel = float((grads[n] - p.grad).norm()) / den
        worst = max(worst, rel)
        assert rel <= TWIN_TOL, (n, rel)
        checked += 1
    print(f"base_encoder: {checked} parameters compared, worst |g - g_twin| / |g_twin| = {worst:.2e}")
    assert checked >= 10
    b3d = [g for n, g in grads.items() if n.startswith("based_3d")]
    assert len(b3d) > 4 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in b3d)


def test_the_gradient_flows_through_the_warp(dev, trained, monkeypatch):
    """With the warp's output detached the encoder's gradients change by more than the twin tolerance: the agreement above is
    not that of two graphs cut at the warp.  (Both steps are reproducible -- two uncut ones agree bit for bit --, so a
    difference is the cut's.)"""
    pristine, frames, targets, _, grads = trained
    cut = copy.deepcopy(pristine)
    real = ops.warp_feature
    with monkeypatch.context() as mp:
        mp.setattr(ops, "warp_feature", lambda *a, **k: real(*a, **k).detach())
        _step(cut, frames, targets)
    cut_grads = _grads(cut)
    moved = []
    for n, g in grads.items():
        if n.startswith("base_encoder") and float(g.norm()) > 0:
            gc = cut_grads.get(n)
            rel = 1.0 if gc is None else float((g - gc).norm()) / float(g.norm())
            if rel > TWIN_TOL:
                moved.append((rel, n))
    print(f"base_encoder parameters whose gradient moves by more than {TWIN_TOL}: {len(moved)}; most: {max(moved) if moved else None}")
    assert moved


def test_base_loss_on_the_feedback_output(dev):
    """As tests/test_fuse_backward.py::test_base_loss_on_the_upsample_output: BaseLoss on a (left, right) pair of outputs."""
    cfg = synth.default_loss_cfg("default_feedback", loss_name="base")
    model = _model(dev, cfg)
    gen = torch.Generator().manual_seed(4)
    T = torch.eye(4)
    T[0, 3] = -0.54
    inputs, targets = _frames(dev), []
    for inp in inputs:
        dc = ops.d_candi_tensor(inp["d_candi"], dev).view(1, -1, 1, 1)
        coarse = 8.0 + 28.0 * torch.rand(B, 1, H // 32, W // 32, generator=gen)
        dmap = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0].to(dev)
        mask = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float().to(dev)
        label = lambda d: torch.softmax(-(dc - d.unsqueeze(1)) ** 2 / (2 * 0.3), dim=1)
        K_up = inp["intrinsics"].clone()
        K_up[:, :2] *= 4.0
        targets.append({"d_candi": inp["d_candi"], "T_left2right": T, "rgb": inp["rgb"], "intrinsics": inp["intrinsics"],
                        "intrinsics_up": K_up, "masks_imgsizes": mask, "masks": mask[:, :, ::4, ::4].contiguous(),
                        "soft_labels_imgsize": label(dmap), "soft_labels": label(dmap[:, ::4, ::4].contiguous())})
    output = tuple(model(inputs))
    assert len(output[0]["output"]) == 2 and len(output[1]["output"]) == 2
    loss = get_loss(cfg, 0)(output, tuple(targets))
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    print("BaseLoss on default_feedback:", float(loss.detach()))
    assert bool(torch.isfinite(loss)) and len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)


def test_deterministic_warp_gradient_carries_the_same_bits(dev, trained):
    """sweep_deterministic = True reaches the warp: the gradient arriving at the warp's input (raw, hooked) is bit-equal across
    two identical steps on deep copies.  Scoped as tests/test_det_scatter_gpu.py::test_base_model_sweep_gradient_carries_the_same_bits:
    the convolutions around it are PyTorch's / MIOpen's to make reproducible, and the test, as that caller, sets
    torch.backends.cudnn.deterministic; what reaches the warp's backward is printed."""
    pristine, frames, targets, _, _ = trained
    caught, seen, flags = [], [], []
    real = ops.warp_feature

    def hooked(src, *a, **k):
        flags.append((k.get("differentiable"), k.get("deterministic")))
        assert src.requires_grad
        src.register_hook(lambda g: caught.append(g.detach().clone()))
        out = real(src, *a, **k)
        out.register_hook(lambda g: seen.append(g.detach().clone()))
        return out

    ops.warp_feature = hooked
    try:
        for _ in range(2):
            _step(copy.deepcopy(pristine), frames, targets)
    finally:
        ops.warp_feature = real
    assert flags == [(True, True)] * 4 and len(caught) == 4 and len(seen) == 4
    for i in range(2):   # (hooks fire in backward order: frame 2, then frame 1, of each step)
        print("frame %d: g_out equal %s (max |diff| %.3e of %.3e), g_raw max |diff| %.3e of %.3e"
              % (2 - i, torch.equal(seen[i], seen[2 + i]), float((seen[i] - seen[2 + i]).abs().max()), float(seen[i].abs().max()),
                 float((caught[i] - caught[2 + i]).abs().max()), float(caught[i].abs().max())))
    for i in range(2):
        assert bool(torch.isfinite(caught[i]).all()) and float(caught[i].abs().max()) > 0
        assert torch.equal(caught[i], caught[2 + i])
