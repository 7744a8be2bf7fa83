"""generate_depth of the reference's utils_lib extension (external/utils_lib/python/utils_lib.cpp:86-160) on the device.

Same signature and return value as the pybind11 function the loader calls (kittiloader/kitti.py:697): one scan -> the
z-buffered, occlusion-filtered depth map [height, width] fp32.  A batch goes through ops.lidar_depth directly."""
import numpy as np
import torch

from .. import ops
from ..harness import _lidar_params


def generate_depth(velodata, intr_raw, M_velo2cam, width, height, params):
    """velodata [N,4] (x, y, z, w) or [N,3], intr_raw [3,4] (or [3,3]), M_velo2cam [4,4]; params: a dict or attribute dict with
    "filtering", "upsample" and optionally "filterdiff" (default 1).  numpy arrays of any float dtype are cast to fp32 (the
    reference's binding converts to MatrixXf), run on the current device and come back as numpy; device tensors give a device
    tensor.  upsample != 0 (the beam resampling, no shipped configuration enables it) raises NotImplementedError."""
    filtering, filterdiff = _lidar_params(params)
    as_numpy = not isinstance(velodata, torch.Tensor)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("generate_depth: the HIP path needs a device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = velodata.device

    def dev_f32(a):
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=torch.float32)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).to(dev)

    pts = dev_f32(velodata)
    if pts.dim() != 2:
        raise RuntimeError(f"generate_depth: velodata must be [N,4] or [N,3], got {tuple(pts.shape)}")
    counts = torch.full((1,), pts.shape[0], dtype=torch.int32, device=dev)
    out = ops.lidar_depth(pts.unsqueeze(0), counts, dev_f32(M_velo2cam), dev_f32(intr_raw), width, height,
                          filtering=filtering, filterdiff=filterdiff)["dmap_imgsizes"][0]
    return out.cpu().numpy() if as_numpy else out
