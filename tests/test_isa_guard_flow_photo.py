"""What the compiler made of the fused photometric kernels of the flow loss (no GPU needed: hipcc cross-compiles):
csrc/flow_photo.hip.  Only the kernels' metadata is read from the listing: every kernel -- the forward, the backward and the final
reduction -- runs in wave64, spills no register of either kind, uses no scratch and fits the 64 KiB of static LDS."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")


def _metadata(name):
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc here")
    r = subprocess.run(["make", "-C", CSRC, name + ".s"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(CSRC, name + ".s")).read()
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        block = m.group(0)
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_flow_photo_kernels_no_spills_no_scratch():
    ks = _metadata("flow_photo")
    for part in ("flow_photo_fwd_kernel", "flow_photo_bwd_kernel", "flow_photo_final_kernel"):
        assert len([k for k in ks if part in k]) == 1, (part, sorted(ks))
    assert len(ks) == 3, sorted(ks)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["group_segment_fixed_size"] <= 65536, (name, md)
