"""What the compiler made of the loss kernels (no GPU needed: hipcc cross-compiles): csrc/loss.hip.  Every kernel -- the forward
and the backward in their instantiations (label / from-depth form x planes per lane, the any-shape kernels) and the final
reduction --: no spilled register of either kind, no scratch, no atomic of any kind (the pixel reduction is a workspace of
partial sums added in a fixed order) and no compare-and-swap loop."""
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


def test_loss_kernels_no_spills_no_scratch_no_atomics():
    ks = _kernels(_listing("loss"))
    fwd = [n for n in ks if "soft_ce_vec4_kernel" in n or "soft_ce_scalar_kernel" in n]
    bwd = [n for n in ks if "soft_ce_bwd" in n]
    fin = [n for n in ks if "soft_ce_final_kernel" in n]
    assert (len(fwd), len(bwd), len(fin)) == (8, 8, 1) and len(ks) == 17, sorted(ks)
    for name, (md, ops) in ks.items():
        assert md["wavefront_size"] == 64, name
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert not [o for o in ops if o.startswith("scratch_")], name
        assert not [o for o in ops if "atomic" in o or "cmpswap" in o or o.startswith(("ds_add", "ds_cmpst"))], name
    for name in fwd + bwd:   # the volume moves in 16-byte accesses in the wave-layout kernels
        if "vec4" in name:
            ops = ks[name][1]
            assert "global_load_dwordx4" in ops, name
            if "bwd" in name:
                assert "global_store_dwordx4" in ops, name
