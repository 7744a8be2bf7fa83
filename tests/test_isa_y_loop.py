"""The waits of the sweep's Y loop, read off the listing (no GPU needed: hipcc cross-compiles).

A wave keeps one register set of operand chunks per block in flight and refills every chunk with the next block's
operands right behind the chunk's last multiplication (csrc/sweep_dist.hip: `fetch`).  The refills
of block j + 1 then have a whole block's time to return -- as long as no `s_waitcnt vmcnt(n)` of the loop asks for a load
that was issued in the same iteration.  vmcnt retires in order: with k operand loads issued so far in the iteration, a wait
with n < k waits for one of them.

The compiler places these waits.  With the refills behind a uniform `if (more)` in the loop body it took, at every join,
the count of the path that issues nothing: the loop of `sweep_dist_kernel<2,1>` read vmcnt(4), (3), (2), (1), (0) with a
refill behind each, and this test FAILS on that listing at `vmcnt(1)` behind three refills (and again at `vmcnt(0)` behind
four; `<.,2>` likewise).  It PASSES on the loop as it is now -- a steady loop in which `more` is a compile-time `true`,
the last blocks of a wave peeled off behind it: vmcnt(4), (3), (4), (4), (4) in `<2,1>`."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")

MFMA = "v_mfma_f32_16x16x32_f16"
LOAD = "buffer_load_dwordx4 v["   # an operand load into registers (the Q records' loads go to LDS: `buffer_load_dwordx4 v84, ... lds`)


@pytest.fixture(scope="module")
def listing():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc here")
    r = subprocess.run(["make", "-C", CSRC, "sweep_dist.s"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(CSRC, "sweep_dist.s")).read()


def kernel_bodies(listing):
    """(NCHK, NH) -> the kernel's lines (labels and instructions, comments stripped)"""
    out = {}
    for m in re.finditer(r"^(_ZN\S*sweep_dist_kernelILi(\d)ELi(\d)E\S*):", listing, re.M):
        end = listing.index("s_endpgm", m.end())
        lines = [l.split(";")[0].strip() for l in listing[m.end():end].split("\n")]
        out[(int(m.group(2)), int(m.group(3)))] = [l for l in lines if l and not l.startswith(".") or re.match(r"\.LBB\d+_\d+:", l)]
    return out


def y_loops(lines):
    """the innermost loops (label .. backward branch to it) that hold both a multiplication and an operand load"""
    label_at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = set()
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)$", l)
        if m and label_at.get(m.group(1), i + 1) <= i:
            loops.add((label_at[m.group(1)], i))
    both = [(a, b) for a, b in loops if any(MFMA in l for l in lines[a:b]) and any(l.startswith(LOAD) for l in lines[a:b])]
    return [(a, b) for a, b in both if not any((c, d) != (a, b) and a <= c and d <= b for c, d in both)]


def same_iteration_waits(body):
    """[(k, n)] of every `s_waitcnt vmcnt(n)` that stands behind k > n operand loads of the iteration"""
    bad, k = [], 0
    for l in body:
        if l.startswith(LOAD):
            k += 1
        m = re.match(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", l)
        if m and int(m.group(1)) < k:
            bad.append((k, int(m.group(1))))
    return bad


def test_no_wait_of_the_y_loop_asks_for_a_load_of_its_own_iteration(listing):
    ks = kernel_bodies(listing)
    assert sorted(ks) == [(c, h) for c in range(3) for h in (1, 2)], sorted(ks)
    for (nchk, nh), lines in sorted(ks.items()):
        loops = y_loops(lines)
        # (the compiler may emit the loop more than once: two copies at NH == 2)
        assert loops, ((nchk, nh), "no loop multiplies and refills")
        ns, nac = nh, 2 * nchk + 1
        for a, b in loops:
            body = lines[a:b + 1]
            # the whole steady state: every chunk of every register set multiplied and refilled once per iteration
            assert sum(l.startswith(LOAD) for l in body) == ns * nac, ((nchk, nh), body)
            assert sum(MFMA in l for l in body) == ns * (3 * nchk + 1), ((nchk, nh), body)
            waits = [l for l in body if re.match(r"s_waitcnt\b.*\bvmcnt\(", l)]
            print((nchk, nh), "waits of the loop:", waits)
            assert waits, (nchk, nh)
            assert same_iteration_waits(body) == [], ((nchk, nh), "(loads issued, vmcnt asked for)", same_iteration_waits(body), body)
