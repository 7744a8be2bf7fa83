"""The lane exchanges of the sweep's reductions and the fold of its row table, read off the listing (no GPU needed: hipcc
cross-compiles).

A `-DDIST_MARKS` build leaves a comment `; MARK i` where the phase stamp i of the kernel stands (csrc/sweep_dist_knobs.hpp).
Between marks 2 and 3 lie the centring and the row table, between 9 and 10 the cost stores and the partial softmax.

1. The centring and the partial softmax reduce over the four K-slice lanes of a pixel: lanes l, l ^ 16, l ^ 32, l ^ 48.
   `quad_sum` / `quad_max` (csrc/wave_util.hpp) carry them by the LDS pipe (`ds_swizzle` / `ds_bpermute`: the product) or, with
   `-DDIST_LANE_XCHG=1`, by the vector pipe (`v_permlane16_swap_b32` / `v_permlane32_swap_b32`).  The swap build is measured
   (profiles/r15_lane_exchange/: no gain in this kernel) and kept buildable: in all six instantiations neither range may hold
   a `ds_swizzle_b32` or a `ds_bpermute_b32`, each holds at least one swap of either width, and the build meets the limits
   tests/test_isa_guard.py sets for the product (nothing spilled, the registers and the LDS of the launch bounds).  (The
   per-batch-item tables in front of mark 2 keep their LDS-pipe shuffles: a few runs per launch; so do the true permutes by
   index of the slots and of the cut, behind mark 4.)
2. The product folds a thread's last update of the row table over groups of eight lanes with DPP (DIST_ROWTAB_FOLD): the three
   chains of three DPP steps stand between marks 2 and 3 of every instantiation, in front of the table's `ds_min_i32` /
   `ds_max_i32`."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm",
         "-amdgpu-atomic-optimizer-strategy=None", "-Wno-unused-function", "-Wno-inline-asm"]
RANGES = {"centring": (2, 3), "partial softmax": (9, 10)}


def _listing(tmp_path_factory, name, *defines):
    if shutil.which("make") is None or not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path_factory.mktemp(name) / "sweep_dist_marks.s")
    r = subprocess.run([HIPCC, *FLAGS, "-DDIST_MARKS", *defines, "-S", "--cuda-device-only", os.path.join(CSRC, "sweep_dist.hip"), "-o", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


@pytest.fixture(scope="module")
def swap_listing(tmp_path_factory):
    return _listing(tmp_path_factory, "swaps", "-DDIST_LANE_XCHG=1")


@pytest.fixture(scope="module")
def product_listing(tmp_path_factory):
    return _listing(tmp_path_factory, "product")


def kernel_bodies(listing):
    """(NCHK, NH) -> the kernel's lines in the order of the listing: instructions, labels and `; MARK i`"""
    out = {}
    for m in re.finditer(r"^(_ZN\S*sweep_dist_kernelILi(\d)ELi(\d)E\S*):", listing, re.M):
        end = listing.index(".Lfunc_end", m.end())   # (a kernel may end in more than one place)
        lines = [l.strip() for l in listing[m.end():end].split("\n")]
        lines = [l if l.startswith("; MARK ") else l.split(";")[0].strip() for l in lines]
        out[(int(m.group(2)), int(m.group(3)))] = [l for l in lines if l and (not l.startswith(".") or re.match(r"\.LBB\d+_\d+:$", l))]
    return out


def between(lines, a, b):
    """The opcodes that can run between a `; MARK a` and a `; MARK b` with no other mark on the way: the instructions reachable
    from a mark a AND from which a mark b is reachable, along the kernel's branches.  (The order of the listing is not the order
    of execution: the compiler lays cold blocks of the Y loop out behind mark 9; and at D > 64 the two passes of a block are two
    copies of the pass, the first copy's mark 9 is followed by the second's mark 2.)"""
    label_at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    mark = {i: int(l.split()[2]) for i, l in enumerate(lines) if l.startswith("; MARK ")}
    succ = [[] for _ in lines]
    for i, l in enumerate(lines):
        op = l.split()[0]
        assert op not in ("s_setpc_b64", "s_swappc_b64"), l   # (no indirect branches: the walk below would miss their targets)
        if op == "s_branch":
            succ[i] = [label_at[l.split()[1]]]
        elif op.startswith("s_cbranch"):
            succ[i] = [label_at[l.split()[1]], i + 1]
        elif op != "s_endpgm" and i + 1 < len(lines):
            succ[i] = [i + 1]
    pred = [[] for _ in lines]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)

    def walk(starts, edges):
        seen, todo = set(), [j for i in starts for j in edges[i]]
        while todo:
            i = todo.pop()
            if i in seen or i in mark:
                continue
            seen.add(i)
            todo.extend(edges[i])
        return seen

    region = walk([i for i, k in mark.items() if k == a], succ) & walk([i for i, k in mark.items() if k == b], pred)
    return [lines[i].split()[0] for i in sorted(region) if not lines[i].endswith(":")]


def test_the_swap_build_crosses_lanes_on_the_vector_pipe(swap_listing):
    ks = kernel_bodies(swap_listing)
    assert sorted(ks) == [(c, h) for c in range(3) for h in (1, 2)], sorted(ks)
    for key, lines in sorted(ks.items()):
        for what, (a, b) in RANGES.items():
            ops = between(lines, a, b)
            assert ops, (key, what, "marks not found")
            lds = [o for o in ops if o.startswith(("ds_swizzle_b32", "ds_bpermute_b32"))]
            assert not lds, (key, what, lds)
            # (the listing writes the encoding behind the name: v_permlane16_swap_b32_e32)
            n16 = sum(o.startswith("v_permlane16_swap_b32") for o in ops)
            n32 = sum(o.startswith("v_permlane32_swap_b32") for o in ops)
            print(key, what, len(ops), "instructions, permlane16_swap", n16, "permlane32_swap", n32)
            assert n16 >= 1 and n32 >= 1, (key, what, sorted(set(ops)))


def test_the_swap_build_keeps_the_product_s_limits(swap_listing):
    seen = 0
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", swap_listing, re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        if "sweep_dist_kernel" not in name:
            continue
        seen += 1
        md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", m.group(0), re.M)}
        assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (name, md)
        nh = int(re.search(r"sweep_dist_kernelILi\dELi(\d)E", name).group(1))
        if nh == 1:
            assert md["vgpr_count"] <= 128 and md["group_segment_fixed_size"] <= 40 * 1024, (name, md)
        else:
            assert md["vgpr_count"] <= 168 and md["group_segment_fixed_size"] <= 53 * 1024, (name, md)
    assert seen == 6, seen
    ops = [l.split()[0] for l in swap_listing.split("\n") if l.strip() and not l.strip().startswith((";", "."))]
    assert not [o for o in ops if re.match(r"v_pk_\w+_f32", o)]


def test_the_product_folds_the_row_table_in_front_of_its_atomics(product_listing):
    ks = kernel_bodies(product_listing)
    assert sorted(ks) == [(c, h) for c in range(3) for h in (1, 2)], sorted(ks)
    for key, lines in sorted(ks.items()):
        body = [l for l in lines if not l.endswith(":")]
        ops = between(lines, 2, 3)
        # (the opcodes alone do not tell a DPP step from another: count the lines of the range's stretch of the listing)
        folds = [l for l in body if re.match(r"v_(min|max)_i32_dpp .* row_half_mirror ", l)]
        # three per pass for the fold (row, least and greatest texel), one each in the two wave reductions behind it
        passes = 2 if key[1] == 2 else 1
        print(key, "row_half_mirror steps:", len(folds), "table atomics in the range:", sum(o in ("ds_min_i32", "ds_max_i32") for o in ops))
        assert len(folds) >= 5 * passes, (key, len(folds))
        assert "ds_min_i32" in ops and "ds_max_i32" in ops, key
        # the product's exchanges: the LDS pipe
        for what, (a, b) in RANGES.items():
            r = between(lines, a, b)
            assert any(o.startswith("ds_swizzle_b32") for o in r) and not any(o.startswith("v_permlane") for o in r), (key, what)
