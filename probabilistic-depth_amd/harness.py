"""Evaluation harness: the counterpart of DefaultTrainer._validate_with_gt for the hot path.

Reproduces the model call + depth regression of the reference's eval loop
(trainer/default_trainer.py:171-321): ``model([inp])[0]`` -> ``prev_output = interpolate(output_refined[-1],
0.25, 'nearest')`` (:221) -> per item ``dpv_to_depthmap(output[-1][b])`` and
``dpv_to_depthmap(output_refined[-1][b])`` (:229-233) -- with the per-item Python loop replaced by one
batched expectation launch per resolution -- and the ground-truth metrics behind it (:243-274): validate_step /
validate compute the devkit's nine depth errors of both resolutions and the uncertainty-field error on the device
(ops.depth_metrics) and read back once, at the end of the trajectory.  Dataset IO and visualisation are out of scope
(SURVEY.md section 2 rows 13-15).
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import ops


def move_input(model_input, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in model_input.items()}


def _model_step(model, model_input, prev_output):
    """The model call of one frame -> (output dict, depth_lowres | None, depth_refined | None, next prev_output)."""
    model_input = dict(model_input)
    model_input["prev_output"] = prev_output
    out = model([model_input])[0]
    # the host model's DPV passes leave the depth maps and the next prev_output behind (one pass over each volume
    # instead of three); any other model gets the reference's op sequence
    aux = getattr(model, "last_aux", None) or {}
    nxt = aux.get("prev_output")
    if nxt is None:
        nxt = F.interpolate(out["output_refined"][-1].detach(), scale_factor=0.25, mode="nearest")
    return out, aux.get("depth_lowres"), aux.get("depth_refined"), nxt


@torch.no_grad()
def eval_step(model, model_input, prev_output=None):
    """One frame of the eval loop.  Returns dict(output, depth_lowres [B,h,w], depth_refined [B,H,W],
    prev_output [B,D,h,w] for the next frame)."""
    out, low, ref, nxt = _model_step(model, model_input, prev_output)
    d_candi = model_input["d_candi"]
    return {
        "output": out,
        "depth_lowres": low if low is not None else ops.dpv_expect(out["output"][-1], d_candi, BV_log=True),
        "depth_refined": ref if ref is not None else ops.dpv_expect(out["output_refined"][-1], d_candi, BV_log=True),
        "prev_output": nxt,
    }


@torch.no_grad()
def eval_trajectory(model, frames):
    """Chained frames of one trajectory (prev_output fed back, reset at frame 0: default_trainer.py:200-202)."""
    prev, results = None, []
    for inp in frames:
        r = eval_step(model, inp, prev)
        prev = r["prev_output"]
        results.append(r)
    return results


@torch.no_grad()
def validate_step(model, model_input, gt_input, prev_output=None, cfg=None):
    """eval_step plus the ground-truth metrics of the frame (trainer/default_trainer.py:229-257), all on the device.

    gt_input: the reference's ground-truth dict -- dmaps [B,h,w], dmap_imgsizes [B,H,W], masks [B,1,h,w], masks_imgsizes
    [B,1,H,W] and, for the uncertainty-field error, soft_labels_imgsize (B volumes [D,H,W]); model_input["intrinsics_up"]
    [B,3,3] is read for that error too.  The truth is clamped at the last depth candidate and the prediction masked inside
    ops.depth_metrics; where the model left its depth maps behind (last_aux) they are the prediction, otherwise the log-DPV is
    (the expectation and the errors from one read of the volume).  With `cfg` (its data.dataset_path picks the parameters of the
    field) the uncertainty-field error of every item is computed as well.  Returns eval_step's dict plus errors [B,9],
    errors_refined [B,9], count [B], count_refined [B] and rmse_unc [B] | None -- tensors: nothing is read back."""
    from .utils import img_utils
    out, low, ref, nxt = _model_step(model, model_input, prev_output)
    d_candi = model_input["d_candi"]
    clamp = float(d_candi[-1])
    res = {"output": out, "prev_output": nxt}
    for key, tag, depth, volume, truth, mask in (
            ("errors", "", low, out["output"][-1], gt_input["dmaps"], gt_input["masks"]),
            ("errors_refined", "_refined", ref, out["output_refined"][-1], gt_input["dmap_imgsizes"], gt_input["masks_imgsizes"])):
        if depth is not None:
            errs, count, _ = ops.depth_metrics(truth, pred=depth, mask=mask, clamp_max=clamp)
        else:
            errs, count, depth = ops.depth_metrics(truth, logp=volume, d_candi=d_candi, mask=mask, clamp_max=clamp, want_depth=True)
        res[key], res["count" + tag] = errs, count
        res["depth_refined" if tag else "depth_lowres"] = depth
    res["rmse_unc"] = None
    if cfg is not None:
        unc = []
        refined = out["output_refined"][-1]
        for b in range(refined.shape[0]):
            truth_f, pred_f, _ = img_utils.compute_unc_field(refined[b:b + 1], gt_input["soft_labels_imgsize"][b].unsqueeze(0), d_candi,
                                                             model_input["intrinsics_up"][b:b + 1], gt_input["masks_imgsizes"][b], cfg)
            unc.append(img_utils.compute_unc_rmse(truth_f, pred_f, d_candi))
        res["rmse_unc"] = torch.stack(unc)
    return res


@torch.no_grad()
def validate(model, frames, cfg=None, sync_debug="error"):
    """The evaluation of one trajectory: frames = [(model_input, gt_input), ...] on the device, prev_output chained as in
    eval_trajectory.  Returns {"rmse", "rmse_refined", "sil", "sil_refined", "rmse_unc", "results", "results_refined"} as
    trainer/default_trainer.py:266-274 forms them (eval_errors over every item of every frame; rmse_unc the mean of the
    per-item uncertainty-field errors, None without `cfg`), plus "steps", the per-frame dicts of validate_step.  The loop
    itself never waits for the device: it runs under torch.cuda.set_sync_debug_mode(sync_debug) -- "error" unless the caller's
    model is known to synchronise --, and the per-item errors of the whole trajectory are read back in one copy at the end.
    An item without a valid pixel raises there, where the reference throws inside its loop."""
    from .utils import img_utils
    frames = list(frames)
    prev, steps = None, []
    if frames:   # the depth candidates are uploaded once per run and cached: a host-to-device copy, so before the loop
        ops.d_candi_tensor(frames[0][0]["d_candi"], frames[0][1]["dmaps"].device)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(sync_debug)
    try:
        for model_input, gt_input in frames:
            r = validate_step(model, model_input, gt_input, prev, cfg)
            prev = r["prev_output"]
            steps.append(r)
        cols = [torch.cat([r["errors"] for r in steps]), torch.cat([r["errors_refined"] for r in steps]),
                torch.cat([r["count"] for r in steps]).unsqueeze(1), torch.cat([r["count_refined"] for r in steps]).unsqueeze(1)]
        if cfg is not None:
            cols.append(torch.cat([r["rmse_unc"] for r in steps]).unsqueeze(1))
        table = torch.cat(cols, dim=1)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    table = table.cpu().numpy()   # the one read-back
    if (table[:, 18:20] == 0).any():
        raise RuntimeError("validate: an item has no valid pixel (its prediction is nowhere > 0 under the mask)")
    results = img_utils.eval_errors([row[:9].tolist() for row in table])
    results_refined = img_utils.eval_errors([row[9:18].tolist() for row in table])
    return {"rmse": results["rmse"][0], "rmse_refined": results_refined["rmse"][0],
            "sil": results["scale invariant log"][0], "sil_refined": results_refined["scale invariant log"][0],
            "rmse_unc": float(np.mean(table[:, 20].astype(np.float64))) if cfg is not None else None,
            "results": results, "results_refined": results_refined, "steps": steps}


@torch.no_grad()
def validate_flow(model, batches, sync_debug="error"):
    """The evaluation of a flow network (the loop of trainer/sintel_trainer.py:92-151): batches = [(img_pair [B,6,H,W], gt_flow
    [B,2|4,Hg,Wg][, move_mask [B,Hg,Wg]]), ...] on the device.  Per batch model(img_pair)['flows_fw'][0] is rescaled, resized
    and compared with the truth by ops.flow_metrics.  Returns {"errors": {name: mean over every item of every batch}, "names",
    "steps"}: names = the columns the truth defines, in the order of ops.FLOW_METRIC_NAMES (evaluate_flow's values first), the
    mean what AverageMeter.update(es, B) accumulates (sintel_trainer.py:121-122); steps = the per-batch {"flow", "errors" [B,8],
    "counts" [B,5]} tensors.  As in validate the loop never waits for the device -- it runs under
    torch.cuda.set_sync_debug_mode(sync_debug) -- and the per-item table is read back in one copy at the end."""
    batches = list(batches)
    steps = []
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(sync_debug)
    try:
        for batch in batches:
            img_pair, gt_flow = batch[0], batch[1]
            flow = model(img_pair)["flows_fw"][0]
            errs, counts, _ = ops.flow_metrics(gt_flow, flow, move_mask=batch[2] if len(batch) > 2 else None)
            steps.append({"flow": flow, "errors": errs, "counts": counts})
        table = torch.cat([s["errors"] for s in steps]) if steps else None
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if table is None:
        raise RuntimeError("validate_flow: no batch to evaluate")
    table = table.cpu().numpy().astype(np.float64)   # the one read-back
    n = 1 if batches[0][1].shape[1] == 2 else (4 if len(batches[0]) < 3 else 8)
    names = ops.FLOW_METRIC_NAMES[:n]
    return {"errors": {name: float(table[:, j].mean()) for j, name in enumerate(names)}, "names": names, "steps": steps}


def _lidar_params(params):
    """(filtering, filterdiff) of the reference's parameter dict / attribute dict; upsample != 0 is refused."""
    get = params.get if hasattr(params, "get") else (lambda k, d=None: getattr(params, k, d))
    if float(get("upsample", 0) or 0) != 0:
        raise NotImplementedError("lidar: params['upsample'] != 0 selects the beam resampling upsample_velodyne "
                                  "(external/utils_lib/python/utils_lib.cpp:20-84), which is not implemented")
    filterdiff = get("filterdiff", None)
    return int(get("filtering")), 1.0 if filterdiff is None else float(filterdiff)


def targets_from_lidar(points, counts, M_velo2cam, intr, width, height, params=None):
    """The ground-truth part of gt_input for a batch of LiDAR scans on the device (kittiloader/kitti.py:683-729): the dict of
    ops.lidar_depth -- dmaps, dmap_imgsizes, masks, masks_imgsizes -- as validate_step and BaseLoss(labels_from_depth=True) read
    them.  params: the loader's {"filtering", "upsample"[, "filterdiff"]}; None = {"filtering": 2, "upsample": 0}, what the loader
    uses when cfg.lidar.enabled is false."""
    filtering, filterdiff = _lidar_params({"filtering": 2, "upsample": 0} if params is None else params)
    return ops.lidar_depth(points, counts, M_velo2cam, intr, width, height, filtering=filtering, filterdiff=filterdiff)


def model_from_config(path, device, id=0):
    """get_model() for an experiment file in the reference's JSON schema (train.py:34-37 + models/get_model.py:4-13):
    returns (model on `device` in eval mode, cfg, the float64 depth candidates of default_trainer.py:38-39)."""
    from . import synth
    from .models import get_model
    cfg = synth.cfg_from_json(path)
    model = get_model(cfg, id).to(device).eval()
    return model, cfg, synth.sweep_workload(cfg)["d_candi"]
