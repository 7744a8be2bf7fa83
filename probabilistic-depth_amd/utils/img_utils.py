"""Drop-in for the hot-path functions of the reference's utils/img_utils.py."""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops


def dpv_to_depthmap(dpv, d_candi, BV_log=False):
    """E[d] of a [1,D,H,W] (log-)DPV -> [1,H,W]  (utils/img_utils.py:52-61)."""
    if dpv.shape[0] != 1:
        raise Exception("Unable to handle this case")
    return ops.dpv_expect(dpv, d_candi, BV_log=BV_log)


def depth_error(predicted, truth):
    """The KITTI devkit's nine depth errors of one depth map against its ground truth -> list of nine floats in the order of
    ops.DEPTH_METRIC_NAMES (utils/img_utils.py:17-22 -> depthError, external/deval_lib/src/evaluate_depth.h:20-121).

    predicted, truth: [H,W] float arrays as the reference's evaluation loop passes them (uploaded to the current device), or
    tensors (device tensors are used where they are).  A zero in either map stands for "no value".  As in the reference the
    arguments reach depthError(D_gt, D_ipol) in this order: a pixel counts where `predicted` is > 0, and the two relative errors
    divide by `predicted`.  Computed by ops.depth_metrics; the only host work is reading the ten numbers back.  Raises
    RuntimeError where the reference throws: no valid pixel."""
    def dev(a):
        if isinstance(a, torch.Tensor):
            return a.float()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    predicted, truth = dev(predicted), dev(truth)
    if predicted.dim() != 2 or predicted.shape != truth.shape:
        raise RuntimeError("depth_error: predicted and truth must be [H,W] maps of one size")   # (the reference: "Wrong file size!")
    metrics, count, _ = ops.depth_metrics(truth.unsqueeze(0), pred=predicted.unsqueeze(0))
    row = torch.cat((metrics[0], count)).tolist()
    if row[9] == 0:
        raise RuntimeError("depth_error: no valid pixel (the prediction is nowhere > 0)")
    return row[:9]


def eval_errors(errors):
    """{name: [mean, min, max]} over a list of depth_error results (utils/img_utils.py:14-15 -> evaluateErrors,
    external/deval_lib/src/evaluate_depth.h:123-142; external/deval_lib/src/utils.h:24-53).  Plain host code.  As in the
    reference the mean is accumulated in float32 in list order, the minimum starts at 1 and the maximum at 0: a metric whose
    values all exceed 1 reports a minimum of 1, and a NaN never replaces either."""
    if len(errors) == 0:
        raise RuntimeError("eval_errors: no errors to evaluate")
    f32 = np.float32
    results = {}
    for i, name in enumerate(ops.DEPTH_METRIC_NAMES[:len(errors[0])]):
        mean, lo, hi = f32(0), f32(1), f32(0)
        for e in errors:
            v = f32(e[i])
            mean = f32(mean + v)
            if v < lo:
                lo = v
            if v > hi:
                hi = v
        results[name] = [float(f32(mean / f32(len(errors)))), float(lo), float(hi)]
    return results


def gaussian_torch(x, mu, sig, pow=2.):
    """exp(-|x - mu|^pow / (2 sig^pow)) (utils/img_utils.py:24-25); sig is a tensor."""
    return torch.exp(-torch.pow(torch.abs(x - mu), pow) / (2 * torch.pow(sig, pow)))


def gen_soft_label_torch(d_candi, depthmap, variance, zero_invalid=False, pow=2.):
    """Soft label [D,H,W] of a depth map [H,W]: a Gaussian of variance `variance` (a tensor) around the depth, evaluated at the
    candidates and normalised over them (utils/img_utils.py:31-47).  A pixel whose Gaussians all underflow divides 0 by 0:
    NaN on every plane, or -1 with zero_invalid.  A torch composition for the data loader's side; the loss itself forms the
    label inside its kernel (ops.dpv_soft_ce(depth_gt=...)) and needs no such tensor."""
    planes = torch.as_tensor(np.asarray(d_candi), dtype=torch.float32).to(depthmap.device).reshape(-1, 1, 1)
    dists = gaussian_torch(planes.expand(-1, depthmap.shape[0], depthmap.shape[1]), depthmap, torch.sqrt(variance), pow)
    dists = dists / torch.sum(dists, dim=0)
    if zero_invalid:
        dists = torch.where(torch.isnan(dists), torch.full_like(dists, -1.0), dists)
    return dists


def minpool(tensor, scale, default=0):
    """Minimum over scale x scale blocks (utils/img_utils.py:87-95); with `default`, zeros stand for "no value": they are
    lifted to `default` before the pooling and blocks that held nothing else come back as 0."""
    if default:
        lifted = torch.where(tensor == 0, torch.full_like(tensor, default), tensor)
        small = -F.max_pool2d(-lifted, scale)
        return torch.where(small == default, torch.zeros_like(small), small)
    return -F.max_pool2d(-tensor, scale)


def powerf(d_min, d_max, nDepth, power):
    """Depth candidates, float64 (utils/img_utils.py:80-85)."""
    x = np.power(np.linspace(start=0, stop=1, num=nDepth), power)
    return np.array([d_min + (d_max - d_min) * v for v in x])


def gen_ufield(dpv_predicted, d_candi, intr_up, visualizer=None, img=None, BV_log=True, normalize=False, mask=None,
               cfg=None, cfgx=None):
    """Uncertainty field of a [1,D,H,W] (log-)DPV -> (plane [1,D,W], masked depth map [1,H,W]).

    Same signature and parameter branches as utils/img_utils.py:268-358: cfgx = {"unc_ang", "unc_shift", "unc_span"}
    (min depth 3, quash on), or cfg.data.dataset_path containing "kitti" (5 rows, band [0.6, 0.9], no quash) or "ilim"
    (no shift, band [1.0, 1.3], min depth 3, quash).  visualizer / img are accepted and unused, like in the reference."""
    if dpv_predicted.shape[0] != 1:
        raise Exception("Unable to handle this case")
    if cfgx is not None:
        pshift, zstart, zend, mind, quash = cfgx["unc_ang"], cfgx["unc_shift"], cfgx["unc_shift"] + cfgx["unc_span"], 3., True
    elif "kitti" in cfg.data.dataset_path:
        pshift, zstart, zend, mind, quash = 5, 0.6, 0.6 + 0.3, 0., False
    elif "ilim" in cfg.data.dataset_path:
        pshift, zstart, zend, mind, quash = 0, 1.0, 1.0 + 0.3, 3., True
    else:
        raise UnboundLocalError("gen_ufield: dataset_path names neither kitti nor ilim")  # the reference fails the same way
    plane, depth_zero = ops.ufield(dpv_predicted, d_candi, intr_up.reshape(1, 3, 3), mask, BV_log=BV_log, unc_ang=pshift,
                                   z_start=zstart, z_end=zend, min_depth=mind, quash=quash)
    if normalize:
        minval, _ = plane.min(1)
        maxval, _ = plane.max(1)
        plane = (plane - minval) / (maxval - minval)
    return plane, depth_zero


def compute_unc_field(dpv_refined_predicted, dpv_refined_truth, d_candi, intr_refined, mask_refined, cfg):
    """(field of the ground-truth DPV, field of the predicted log-DPV, masked depth map of the prediction)
    (utils/img_utils.py:178-181; called by the evaluation loop, trainer/default_trainer.py:243-244): two gen_ufield
    collapses through the dataset branch of `cfg` -- the truth as probabilities under its validity mask, the prediction as
    a log-DPV without one.  intr_refined [1,3,3]."""
    unc_field_truth, _ = gen_ufield(dpv_refined_truth, d_candi, intr_refined.squeeze(0), BV_log=False, mask=mask_refined, cfg=cfg)
    unc_field_predicted, debugmap = gen_ufield(dpv_refined_predicted, d_candi, intr_refined.squeeze(0), BV_log=True, cfg=cfg)
    return unc_field_truth, unc_field_predicted, debugmap


def compute_unc_rmse(unc_field_truth, unc_field_predicted, d_candi, plot=False):
    """Error between two [1,D,W] uncertainty fields (utils/img_utils.py:183-202): E[d] per column of each, the
    predicted one zeroed in the first and last column, columns where either is NaN (no qualifying pixel) dropped.
    Despite the name the value returned is the mean absolute difference -- the reference overwrites its RMSE with it
    (:192-193).  `plot` is accepted and ignored (the reference draws the two curves with matplotlib)."""
    import torch
    truth_depth = dpv_to_depthmap(unc_field_truth.unsqueeze(2), d_candi, BV_log=False).squeeze(0).squeeze(0)
    pred_depth = dpv_to_depthmap(unc_field_predicted.unsqueeze(2), d_candi, BV_log=False).squeeze(0).squeeze(0)
    pred_depth[0].zero_()    # (in place on the views: `pred_depth[0] = 0` uploads its scalar and waits for the device)
    pred_depth[-1].zero_()
    usable = ~torch.isnan(truth_depth) & ~torch.isnan(pred_depth)
    truth_depth = torch.where(usable, truth_depth, torch.zeros_like(truth_depth))
    pred_depth = torch.where(usable, pred_depth, torch.zeros_like(pred_depth))
    return torch.sum(torch.abs(truth_depth - pred_depth)) / torch.sum(usable)
