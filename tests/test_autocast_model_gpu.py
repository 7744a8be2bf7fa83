"""GPU suite: the models under torch.autocast.  The conv stacks then hand fp16 / bf16 logits to the DPV reductions, which widen
them in their load (csrc/dpv_half.hip) and return fp32 log-DPVs; the quarter-resolution tensors that feed fp32-only ops (the
sweep's features, warp_feature's input, the feedback residual) are upcast in the model.  What is checked is that every nmode
runs, that what comes out is an fp32 log-DPV, and that a training step leaves a finite fp32 gradient wherever the fp32 step
leaves one.  No value is compared with the fp32 model: that would be a statement about the half-precision convolutions."""
import pytest
import torch
import torch.nn.functional as F

import pdepth_amd  # noqa: F401
from pdepth_amd import harness, ops, synth
from pdepth_amd.losses.get_loss import get_loss
from pdepth_amd.models.get_model import get_model

pytestmark = pytest.mark.gpu

B, H, W = 1, 256, 256   # a 64 x 64 sweep: the smallest image the encoder takes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


def _input(seed, dev, gen):
    inp = synth.make_model_input(seed, B=B, V=1, H=H, W=W, D=64, pose="mono")
    masks = (torch.rand(B, 1, H // 4, W // 4, generator=gen) > 0.7).float()
    inp["dmaps"] = (torch.rand(B, H // 4, W // 4, generator=gen) * 30 + 6) * masks[:, 0]
    inp["masks"] = masks
    return harness.move_input(inp, dev)


def _model(cfg, dev, train=False):
    torch.manual_seed(0)
    model = get_model(cfg, 0)
    synth.seed_weights(model, seed=31)
    return model.to(dev).train(train)


def _check_log_dpvs(out):
    vols = out["output"] + out["output_refined"]
    assert vols
    for v in vols:
        assert v.dtype == torch.float32 and v.dim() == 4
        assert bool(torch.isfinite(v).all())
        assert torch.logsumexp(v, dim=1).abs().max().item() <= 1e-5


@pytest.mark.parametrize("nmode,model_name", [("default", "base"), ("default_upsample", "base"), ("default_feedback", "base"),
                                              ("default", "default")],
                         ids=["default", "default_upsample", "default_feedback", "DefaultModel"])
def test_inference_under_bf16_autocast(dev, nmode, model_name):
    model = _model(synth.default_cfg(nmode, model_name=model_name), dev)
    gen = torch.Generator().manual_seed(1)
    frames = [_input(3100 + i, dev, gen) for i in range(2 if nmode == "default_feedback" else 1)]
    prev = None
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for inp in frames:   # (the second frame of the feedback model takes the first one's quarter-resolution log-DPV)
            r = harness.eval_step(model, inp, prev)
            prev = r["prev_output"]
            _check_log_dpvs(r["output"])
            assert prev.dtype == torch.float32 and prev.shape[1:] == (64, H // 4, W // 4) and bool(torch.isfinite(prev).all())
            for key, shape in (("depth_lowres", (B, H // 4, W // 4)), ("depth_refined", (B, H, W))):
                d = r[key]
                assert d.dtype == torch.float32 and tuple(d.shape) == shape and bool(torch.isfinite(d).all()), key
                assert d.min().item() >= 5.0 - 1e-3 and d.max().item() <= 40.0 + 1e-3, key


def test_inference_under_fp16_autocast(dev):
    model = _model(synth.default_cfg("default"), dev)
    inp = _input(3100, dev, torch.Generator().manual_seed(1))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = model([inp])[0]
    _check_log_dpvs(out)


def _targets(inp, dev, gen):
    dc = ops.d_candi_tensor(inp["d_candi"], dev).view(1, -1, 1, 1)
    coarse = 8.0 + 28.0 * torch.rand(B, 1, H // 32, W // 32, generator=gen)
    dmap = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0].to(dev)
    mask = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float().to(dev)
    label = lambda d: torch.softmax(-(dc - d.unsqueeze(1)) ** 2 / (2 * 0.3), dim=1)
    T = torch.eye(4)
    T[0, 3] = -0.54
    K_up = inp["intrinsics"].clone()
    K_up[:, :2] *= 4.0
    return {"d_candi": inp["d_candi"], "T_left2right": T, "rgb": inp["rgb"], "intrinsics": inp["intrinsics"],
            "intrinsics_up": K_up, "masks_imgsizes": mask, "masks": mask[:, :, ::4, ::4].contiguous(),
            "soft_labels_imgsize": label(dmap), "soft_labels": label(dmap[:, ::4, ::4].contiguous())}


@pytest.mark.parametrize("nmode", ["default", "default_upsample"])
def test_training_step_under_bf16_autocast(dev, nmode):
    cfg = synth.default_loss_cfg(nmode, loss_name="base")
    model = _model(cfg, dev, train=True)
    gen = torch.Generator().manual_seed(4)
    inputs = [_input(seed, dev, gen) for seed in (3100, 3101)]
    targets = tuple(_targets(inp, dev, gen) for inp in inputs)
    criterion = get_loss(cfg, 0)

    def step(autocast):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            output = tuple(model(inputs))
            loss = criterion(output, targets)
        for out in output:
            for v in out["output"] + out["output_refined"]:
                assert v.dtype == torch.float32
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
        loss.backward()
        return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}

    want = step(False)
    got = step(True)
    assert len(want) > 10
    for n in want:
        assert n in got, n
        assert got[n].dtype == torch.float32 and bool(torch.isfinite(got[n]).all()), n
