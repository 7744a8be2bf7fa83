"""What the compiler made of the DPV reduction kernels (no GPU needed: hipcc cross-compiles): csrc/dpv.hip, read from the
code-object metadata of `make dpv.s` alone.  Every kernel -- the three wave-layout kernels (csrc/dpv_lanes.hpp) in their
instantiations by planes per lane, and the any-shape kernels beside them --: wave size 64, no spilled register of either
kind, no private segment (scratch); each wave-layout kernel within the registers of the waves per SIMD it runs at."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")

# Registers are allocated in steps of 8 per lane out of 512 per lane of a SIMD: at most 64 | 72 | 80 | 96 | 128 | 168 | 256
# of them for 8 | 7 | 6 | 5 | 4 | 3 | 2 waves per SIMD.  (kernel, planes per lane) -> the most it may use to keep its waves:
#   reduce      63 / 103 / 183 registers when this guard was written (the last the tightest kernel of the file)
#   reduce_ex   72 / 120 / 216
#   expect      39 / 72 / 137 (a DPV) and 49 / 78 / 147 (a log-DPV)
VGPR_LIMIT = {
    ("dpv_reduce_vec4_kernel", 8): 64, ("dpv_reduce_vec4_kernel", 16): 128, ("dpv_reduce_vec4_kernel", 32): 256,
    ("dpv_reduce_ex_vec4_kernel", 8): 72, ("dpv_reduce_ex_vec4_kernel", 16): 128, ("dpv_reduce_ex_vec4_kernel", 32): 256,
    ("dpv_expect_vec4_kernel<false>", 8): 64, ("dpv_expect_vec4_kernel<false>", 16): 72, ("dpv_expect_vec4_kernel<false>", 32): 168,
    ("dpv_expect_vec4_kernel<true>", 8): 64, ("dpv_expect_vec4_kernel<true>", 16): 80, ("dpv_expect_vec4_kernel<true>", 32): 168,
}


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


def _vec4_key(mangled):
    """Itanium names: ...dpv_reduce_vec4_kernelILi16EE..., ...dpv_expect_vec4_kernelILb1ELi16EE... -> the key of VGPR_LIMIT."""
    m = re.search(r"(dpv_\w+_vec4_kernel)I(?:Lb([01])E)?Li(\d+)EE", mangled)
    assert m, mangled
    kernel = m.group(1) if m.group(2) is None else "%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")
    return kernel, int(m.group(3))


def test_dpv_kernels_no_spills_no_scratch_and_keep_their_waves():
    ks = _metadata("dpv")
    vec = [n for n in ks if "_vec4_kernel" in n]
    rest = [n for n in ks if "dpv_reduce_scalar_kernel" in n or "dpv_reduce_ex_scalar_kernel" in n or "dpv_expect_kernel" in n]
    # 3 + 3 + 6 wave-layout kernels; the two any-shape reductions and dpv_expect_kernel<BV_LOG, VEC = 1 | 4>
    assert (len(vec), len(rest)) == (12, 6) and len(ks) == 18, sorted(ks)
    for name, md in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 256, (name, md)
    assert sorted(_vec4_key(n) for n in vec) == sorted(VGPR_LIMIT)
    for name in vec:
        assert ks[name]["vgpr_count"] + ks[name]["agpr_count"] <= VGPR_LIMIT[_vec4_key(name)], (name, ks[name]["vgpr_count"])
