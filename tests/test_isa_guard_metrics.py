"""What the compiler made of the evaluation-metrics kernels (no GPU needed: hipcc cross-compiles): csrc/metrics.hip, read from
the code-object metadata of `make metrics.s` alone.  Every kernel -- the wave-layout volume kernel in its three instantiations
(planes per lane), the any-shape volume kernel, the depth map kernel and the final reduction --: wave size 64, no spilled
register of either kind, no private segment (scratch)."""
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


def test_metrics_kernels_no_spills_no_scratch():
    ks = _metadata("metrics")
    vec = [n for n in ks if "depth_metrics_vec4_kernel" in n]
    rest = [n for n in ks if "depth_metrics_scalar_kernel" in n or "depth_metrics_map_kernel" in n or "depth_metrics_final_kernel" in n]
    assert (len(vec), len(rest)) == (3, 3) and len(ks) == 6, sorted(ks)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256, (name, md)
    # the 16 loads of 16 bytes in flight per lane fit with room for four waves per SIMD (512 registers per lane of a SIMD)
    for name in vec:
        assert ks[name]["vgpr_count"] <= 128, (name, ks[name]["vgpr_count"])
