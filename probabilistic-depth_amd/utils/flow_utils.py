"""Drop-in for the evaluation functions of the reference's utils/flow_utils.py: evaluate_flow and resize_flow, computed on the
device by ops.flow_metrics / ops.flow_resize (csrc/flow_metrics.hip).

Out of scope: load_flow and flow_to_image (utils/flow_utils.py:7-47) are host I/O and visualisation and need OpenCV and
matplotlib; they are not provided here."""
import numpy as np
import torch

from .. import ops


def resize_flow(flow, new_shape):
    """flow [B,2,h,w] -> [B,2,new_h,new_w]: bilinear with align_corners=True, u scaled by new_w / w and v by new_h / h
    (utils/flow_utils.py:50-58), one HIP pass (ops.flow_resize(align_corners=True)).  Returns a new tensor and leaves `flow`
    as it is; the reference scales the interpolated tensor in place, which is its own new tensor too."""
    return ops.flow_resize(flow, new_shape, align_corners=True)


def _items(maps, channels_last):
    """A batch as a list of per-item device tensors [C,H,W] (or [H,W] for masks), uploaded where it comes from the host."""
    if isinstance(maps, torch.Tensor):
        if not maps.is_cuda:
            raise RuntimeError(f"evaluate_flow: the HIP path needs a device tensor (got {maps.device}); there is no CPU fallback")
        return list(maps.float())
    out = []
    for m in maps:
        if isinstance(m, torch.Tensor):
            t = m.float().cuda()
        else:
            t = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda()
        out.append(t.permute(2, 0, 1) if channels_last and t.dim() == 3 else t)
    return out


def evaluate_flow(gt_flows, pred_flows, moving_masks=None):
    """The batch means of the flow errors -> list of floats: [epe] for a 2-channel truth, [epe, epe_noc, epe_occ, fl] for a
    4-channel truth (u, v, valid, noc), and with moving_masks also [.., epe_move, epe_static] (utils/flow_utils.py:61-123).

    gt_flows, pred_flows: the reference's lists (or arrays) of [H,W,C] numpy maps, one per item, or device tensors [B,C,H,W];
    moving_masks: a list of [H,W] maps or a tensor [B,H,W].  Every prediction is rescaled and resized to its truth's size by
    cv2.resize's bilinear rule inside ops.flow_metrics; items of differing sizes are evaluated one call per size group.  The
    per-item table stays on the device and is read back once, at the end; the mean over the items is formed in float64 as
    the reference's Python sum is."""
    tensors = isinstance(gt_flows, torch.Tensor)
    gts, preds = _items(gt_flows, not tensors), _items(pred_flows, not isinstance(pred_flows, torch.Tensor))
    moves = None if moving_masks is None else _items(moving_masks, False)
    B = len(gts)
    if B == 0 or len(preds) != B or (moves is not None and len(moves) != B):
        raise RuntimeError("evaluate_flow: gt_flows, pred_flows and moving_masks must hold one map per item, at least one")
    C = gts[0].shape[0]
    if C not in (2, 4) or any(g.shape[0] != C for g in gts):
        raise RuntimeError("evaluate_flow: every truth must have 2 channels (u, v) or 4 (u, v, valid, noc)")
    if C == 2:
        moves = None   # (the reference reads the masks for a 4-channel truth only)
    groups = {}
    for i in range(B):
        groups.setdefault((tuple(gts[i].shape), tuple(preds[i].shape)), []).append(i)
    rows = []
    for idx in groups.values():
        gt = torch.stack([gts[i] for i in idx])
        pred = torch.stack([preds[i][:2] for i in idx])
        move = None if moves is None else torch.stack([moves[i].reshape(gt.shape[2:]) for i in idx])
        rows.append(ops.flow_metrics(gt, pred, move_mask=move)[0])
    table = torch.cat(rows).cpu().numpy().astype(np.float64)   # the one read-back
    n = 1 if C == 2 else (4 if moves is None else 6)
    return [float(table[:, j].sum() / B) for j in (0, 1, 2, 3, 4, 5)[:n]]
