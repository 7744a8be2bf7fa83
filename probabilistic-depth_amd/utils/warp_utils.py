"""Flow-warp helpers with the names and argument lists of the reference's utils/warp_utils.py, so that code written against it
imports unchanged.

get_corresponding_map and get_occu_mask_backward are the HIP range map of csrc/occlusion.hip (ops.range_map, ops.occlusion_mask):
an order-independent integer sum, the same bits from call to call.  flow_warp and get_occu_mask_bidirection on fp32 device tensors
(mode='bilinear') are the HIP kernels of csrc/flow_warp.hip (ops.flow_warp with both gradients, ops.flow_fb_check); everything else
-- CPU tensors, other dtypes, mode='nearest' -- is the plain torch composition around F.grid_sample, as in the reference, and runs
wherever its tensors live.
"""
import torch
import torch.nn.functional as F

from .. import ops


def mesh_grid(B, H, W):
    """Pixel coordinates [B,2,H,W], int64, on the CPU: channel 0 the column x, channel 1 the row y (warp_utils.py:6-12)."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack((xs, ys), 0).unsqueeze(0).repeat(B, 1, 1, 1)


def norm_grid(v_grid):
    """Un-normalised positions [B,2,H,W] -> the [-1, 1] grid [B,H,W,2] of F.grid_sample, 2 x / (W - 1) - 1 (warp_utils.py:15-22)."""
    _, _, H, W = v_grid.shape
    gx = 2.0 * v_grid[:, 0] / (W - 1) - 1.0
    gy = 2.0 * v_grid[:, 1] / (H - 1) - 1.0
    return torch.stack((gx, gy), -1)


def get_corresponding_map(data):
    """Range map [B,1,H,W] of un-normalised positions [B,2,H,W] (warp_utils.py:25-79): ops.range_map, HIP, device tensors only."""
    return ops.range_map(data)


def _on_hip(*tensors):
    """True where the HIP ops take the call: every tensor fp32 and on a device."""
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors)


def flow_warp(x, flow12, pad='border', mode='bilinear'):
    """x [B,C,H,W] sampled at base grid + flow12 (warp_utils.py:82-89).  fp32 device tensors with mode='bilinear': ops.flow_warp,
    HIP, differentiable in x and flow12.  Otherwise a plain torch composition around F.grid_sample with the reference's call
    (align_corners=False, torch's default, which the reference leaves unsaid)."""
    if mode == 'bilinear' and _on_hip(x, flow12):
        return ops.flow_warp(x, flow12, pad=pad)
    B, _, H, W = x.shape
    base = mesh_grid(B, H, W).to(device=x.device, dtype=x.dtype)
    return F.grid_sample(x, norm_grid(base + flow12), mode=mode, padding_mode=pad, align_corners=False)


def get_occu_mask_bidirection(flow12, flow21, scale=0.01, bias=0.5):
    """Forward-backward check (warp_utils.py:92-99): 1 where |flow12 + warp(flow21)|^2 exceeds scale (|flow12|^2 + |warp(flow21)|^2)
    + bias.  fp32 device tensors: ops.flow_fb_check, one HIP pass; otherwise a plain torch composition over flow_warp."""
    if _on_hip(flow12, flow21):
        return ops.flow_fb_check(flow12, flow21, scale=scale, bias=bias)
    back = flow_warp(flow21, flow12, pad='zeros')
    both = flow12 + back
    mag = (flow12 * flow12).sum(1, keepdim=True) + (back * back).sum(1, keepdim=True)
    return ((both * both).sum(1, keepdim=True) > scale * mag + bias).float()


def get_occu_mask_backward(flow21, th=0.2):
    """Occluded mask [B,1,H,W] (1 = no pixel of the other view lands here) of a flow [B,2,H,W] (warp_utils.py:102-108): the base
    grid plus the flow through ops.occlusion_mask, returned as 1 - visible, as the reference returns it."""
    B, _, H, W = flow21.shape
    base = mesh_grid(B, H, W).to(device=flow21.device, dtype=flow21.dtype)
    return 1.0 - ops.occlusion_mask(base + flow21, th=th)
