"""Golden fixture g29_pwclite: the reference's PWCLite (models/pwclite.py) on the CPU, in float32 and in float64, and ten Adam
steps of it under the reference's unFlowLoss.  Build container only (imports the reference, which never travels):

    python tests/golden/make_golden_pwclite.py

The reference's CUDA-only correlation package is aliased to its own models/correlation_native.py (same arithmetic in plain torch)
before models.pwclite is imported; what the reference prints is captured and dropped.  Weights on both sides:
synth.seed_weights(model, seed=29, gain=0.25), keyed by parameter name.  Inputs and cases: tests/util_cost_volume.py (PWC_CASES,
pwc_input, train_pair, train_cfg).

Stored, data only:  state.<reduce|dense|reduce3>  the state-dict names with their shapes ("name:16x3x3x3");  per case and flow
(util_cost_volume.pwc_flows) `<case>.<key>.v64` every k-th element of the float64 flow (pwc_subset), `.err` the reference's own
fp32 error against float64 over EVERY element, `.max` max |flow|;  train.totals32 the ten totals of the float32 trajectory,
train.step0_32 / train.step0_64 the four values of step 0 in both precisions.

Checked here: the conditions on the inputs of the op tests (util_cost_volume.check_conditions); the finest forward flow of every
case has max |flow| between 1 and 32 px (the dense case: 32.2 px whatever the input, see below); this package's PWCLite on the CPU gives the reference's flows to 1e-10 in float64.
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

import util_cost_volume as U  # noqa: E402


def _reference_modules():
    _import_reference()
    import models.correlation_native as native
    sys.modules["models.correlation_package.correlation"] = native
    import models.correlation_package as pkg
    pkg.correlation = native
    import models.pwclite as pwc
    import losses.flow_loss as fl
    return pwc, fl


def _quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def _model(pwc, frames, reduce_dense, dtype):
    from pdepth_amd import synth
    model = pwc.PWCLite(U.pwc_cfg(frames, reduce_dense))
    synth.seed_weights(model, seed=U.PWC_SEED, gain=U.PWC_GAIN)
    return model.to(dtype)


def _state(model):
    return np.array(["%s:%s" % (k, "x".join(str(s) for s in v.shape)) for k, v in model.state_dict().items()])


def main():
    pwc, fl = _reference_modules()
    from pdepth_amd.models import pwclite as mine
    from pdepth_amd import synth
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for case in U.CASES:
            least, share = U.check_conditions(case)
            print(f"{U.case_id(case)}: least |pre-activation| {least:.1f} thresholds, left out of grad_flow {100 * share:.2f} %")

        out["state.reduce"] = _state(pwc.PWCLite(U.pwc_cfg(2, True)))
        out["state.dense"] = _state(pwc.PWCLite(U.pwc_cfg(2, False)))
        out["state.reduce3"] = _state(pwc.PWCLite(U.pwc_cfg(3, True)))
        for (frames, reduce_dense), n in U.PWC_PARAMETERS.items():
            assert pwc.PWCLite(U.pwc_cfg(frames, reduce_dense)).num_parameters() == n, (frames, reduce_dense)

        for name, (frames, reduce_dense, with_bk, B) in U.PWC_CASES.items():
            x = U.pwc_input(name)
            res = {}
            for dtype in (torch.float32, torch.float64):
                with torch.no_grad():
                    res[dtype] = U.pwc_flows(_quiet(_model(pwc, frames, reduce_dense, dtype), x.to(dtype), with_bk=with_bk))
            own = mine.PWCLite(U.pwc_cfg(frames, reduce_dense))
            synth.seed_weights(own, seed=U.PWC_SEED, gain=U.PWC_GAIN)
            with torch.no_grad():
                own64 = U.pwc_flows(own.double()(x.double(), with_bk=with_bk))
            finest = float(dict(res[torch.float64])["fw.0.0" if frames == 5 else "fw.0"].abs().max())
            # a condition on the inputs: flows of a few pixels, neither nothing nor an explosion.  The dense estimator's flow with
            # these weights is set by its biases, 32.20 px at the lower border for any input (measured at 0.25 to 30 times the
            # image's amplitude): no input brings it under 32, so that case is held to the lower bound alone
            assert 1.0 <= finest and (finest <= 32.0 or not reduce_dense), (name, finest)
            worst = 0.0
            for (key, v32), (key64, v64), (key_own, o64) in zip(res[torch.float32], res[torch.float64], own64):
                assert key == key64 == key_own and v32.shape == v64.shape == o64.shape
                assert float((o64 - v64).abs().max()) <= 1e-10 * max(1.0, float(v64.abs().max())), (name, key)
                err = float((v32.double() - v64).abs().max())
                out[f"{name}.{key}.v64"] = U.pwc_subset(v64.numpy())
                out[f"{name}.{key}.err"] = np.float64(err)
                out[f"{name}.{key}.max"] = np.float64(v64.abs().max())
                worst = max(worst, err / float(v64.abs().max()))
            print(f"{name}: {len(res[torch.float64])} flows, finest max |flow| {finest:.2f} px, worst fp32 error / max |flow| {worst:.1e}")

        # the training trajectory: the first case, ten Adam steps under the reference's loss
        target, steps = U.train_pair(), {}
        for dtype in (torch.float32, torch.float64):
            model = _model(pwc, 2, True, dtype)
            loss_fn = fl.unFlowLoss(U.train_cfg())
            opt = torch.optim.Adam(model.parameters(), lr=U.TRAIN_LR)
            rows = []
            for _ in range(U.TRAIN_STEPS if dtype == torch.float32 else 1):
                opt.zero_grad()
                vals = _quiet(loss_fn, U.train_output(_quiet(model, target.to(dtype), with_bk=True)), target.to(dtype))
                rows.append([float(v) for v in vals])
                vals[0].backward()
                opt.step()
            steps[dtype] = np.array(rows, np.float64)
        out["train.totals32"] = steps[torch.float32][:, 0]
        out["train.step0_32"], out["train.step0_64"] = steps[torch.float32][0], steps[torch.float64][0]
        t = out["train.totals32"]
        print("train totals:", " ".join(f"{v:.4f}" for v in t), f"ratio {t[-1] / t[0]:.3f}")
        print("step 0: float32", out["train.step0_32"], "float64", out["train.step0_64"])
    path = os.path.join(HERE, "g29_pwclite.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
