"""What the compiler made of the flow-evaluation kernels (no GPU needed: hipcc cross-compiles): csrc/flow_metrics.hip, read from
the code-object metadata of `make flow_metrics.s` alone.  Every kernel -- the metrics kernel in its six instantiations (three
forms of the truth, 16-byte and scalar fetch), the three final reductions and the resize --: wave size 64, no spilled register
of either kind, no private segment (scratch), a workgroup of 256."""
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


def test_flow_metrics_kernels_no_spills_no_scratch():
    ks = _metadata("flow_metrics")
    for part, n in (("flow_metrics_kernel", 6), ("flow_metrics_final_kernel", 3), ("flow_resize_kernel", 1)):
        assert len([k for k in ks if part in k]) == n, (part, sorted(ks))
    assert len(ks) == 10, sorted(ks)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256, (name, md)
