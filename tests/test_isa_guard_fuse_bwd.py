"""What the compiler made of the DPV fusion backward (no GPU needed: hipcc cross-compiles): csrc/dpv_fuse_bwd.hip.  Every kernel
-- the register form in its instantiations (full / partial depth x gradients present) and the two re-reading kernels --:
wavefront size 64, no spilled register of either kind, no scratch."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")


def _listing(name):
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc here")
    r = subprocess.run(["make", "-C", CSRC, name + ".s"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(CSRC, name + ".s")).read()


def _kernels(text):
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        block = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
        start = text.index("\n" + name + ":")
        end = text.index(".Lfunc_end", start)   # (a kernel may hold more than one s_endpgm: early exits)
        body = [l.strip() for l in text[start:end].split("\n")]
        out[name] = (md, [l.split()[0] for l in body if l and not l.startswith((";", ".")) and not l.endswith(":")])
    return out


def test_fuse_backward_kernels_no_spills_no_scratch():
    ks = _kernels(_listing("dpv_fuse_bwd"))
    reg = [n for n in ks if "dpv_fuse_bwd_reg_kernel" in n]
    any_d = [n for n in ks if "dpv_fuse_bwd_kernel" in n]
    assert (len(reg), len(any_d)) == (6, 2) and len(ks) == 8, sorted(ks)
    for name, (md, ops) in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert not [o for o in ops if o.startswith("scratch_")], name
