"""What the compiler made of the deterministic scatter kernels (no GPU needed: hipcc cross-compiles): csrc/sweep_bwd_det.hip and
csrc/scatter_det.hip.  Every kernel: no spilled register of either kind, no scratch, no compare-and-swap loop; the adds of the
scatter kernels are 64-bit integer atomics -- global_atomic_add_x2 on global memory, ds_add_u64 on the LDS box image of the
sweep -- and none is a float atomic."""
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


def _is_float_atomic(op):
    return ("atomic" in op or op.startswith("ds_add") or op.startswith("ds_pk_add")) and re.search(r"_f(16|32|64)|bf16", op) is not None


@pytest.mark.parametrize("unit,n", [("sweep_bwd_det", 4), ("scatter_det", 7)])
def test_no_spills_no_scratch_no_cmpswap_no_float_atomic(unit, n):
    ks = _kernels(_listing(unit))
    assert len(ks) == n, sorted(ks)
    for name, (md, ops) in ks.items():
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert not [o for o in ops if "cmpswap" in o or "cmpst" in o], (name, "compare-and-swap loop")
        assert not [o for o in ops if _is_float_atomic(o)], (name, "float atomic")


def test_sweep_scatter_adds_are_integer_atomics():
    ks = _kernels(_listing("sweep_bwd_det"))
    scatter = {n: ops for n, (md, ops) in ks.items() if "sweep_bwd_det_kernel" in n}
    assert len(scatter) == 2, sorted(ks)   # L2, L1
    for name, ops in scatter.items():
        assert "global_atomic_add_x2" in ops and "ds_add_u64" in ops, name
        assert not [o for o in ops if "atomic" in o and o != "global_atomic_add_x2"], name
        assert not [o for o in ops if o.startswith("ds_add") and o != "ds_add_u64"], name
    # the pre-pass: an integer maximum over bit patterns; the convert pass: no atomic at all
    (bounds,) = [ops for n, (md, ops) in ks.items() if "bounds_kernel" in n]
    assert [o for o in bounds if "atomic" in o] == ["global_atomic_umax"]
    (convert,) = [ops for n, (md, ops) in ks.items() if "convert_kernel" in n]
    assert not [o for o in convert if "atomic" in o]


def test_image_scatter_adds_are_integer_atomics():
    ks = _kernels(_listing("scatter_det"))
    for name, (md, ops) in ks.items():
        atomics = sorted(set(o for o in ops if "atomic" in o))
        if "convert_kernel" in name:
            assert atomics == [], name
        elif "ILi0EEE" in name or "ELi0EEE" in name:     # <PASS = 0>: the maximum
            assert atomics == ["global_atomic_umax"], (name, atomics)
        else:                                            # <PASS = 1>: the scatter
            assert atomics == ["global_atomic_add_x2"], (name, atomics)
