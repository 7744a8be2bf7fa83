"""What the compiler made of the backward kernels (no GPU needed: hipcc cross-compiles): csrc/sweep_bwd.hip and
csrc/dpv_bwd.hip.  Every kernel: no spilled register of either kind, no scratch, no compare-and-swap loop; the float adds of
the scatter are global_atomic_add_f32 (global memory) and ds_add_f64 (the LDS box image, kept in double: DESIGN.md 6.1.4)."""
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
        end = text.index("s_endpgm", start)
        body = [l.strip() for l in text[start:end].split("\n")]
        out[name] = (md, [l.split()[0] for l in body if l and not l.startswith((";", ".")) and not l.endswith(":")])
    return out


@pytest.mark.parametrize("unit,n", [("sweep_bwd", 4), ("dpv_bwd", 2)])
def test_no_spills_no_scratch_no_cmpswap(unit, n):
    ks = _kernels(_listing(unit))
    assert len(ks) == n, sorted(ks)
    for name, (md, ops) in ks.items():
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert not [o for o in ops if "cmpswap" in o], (name, "compare-and-swap loop")


def test_scatter_adds_are_float_atomics():
    ks = _kernels(_listing("sweep_bwd"))
    scatter = {n: ops for n, (md, ops) in ks.items() if "ELb0ELb1E" in n}   # <METRIC, GREF = false, GSRC = true>
    gather = {n: ops for n, (md, ops) in ks.items() if "ELb1ELb0E" in n}
    assert len(scatter) == 2 and len(gather) == 2, sorted(ks)
    for name, ops in scatter.items():
        assert "global_atomic_add_f32" in ops and "ds_add_f64" in ops, name
        assert not [o for o in ops if o.startswith("ds_add") and o != "ds_add_f64"], name   # (no returning add, no float32 image)
        assert not [o for o in ops if "atomic" in o and o not in ("global_atomic_add_f32",)], name
    for name, ops in gather.items():   # g_ref: a gather, no atomics at all
        assert not [o for o in ops if "atomic" in o or o.startswith("ds_add")], name
