"""The sweep workspace is described once, in csrc/sweep_workspace.hpp, and a workspace packed by an earlier build of ABI 6
must stay valid: the byte offsets of its regions are pinned here to the numbers the library answered before that header
existed.  A stand-alone host program (its own main, no GPU) prints what the header computes; the built library must size
its workspaces by the same totals; and on the device, a pack + sweep writes its layout tag and statistics where the table
says and nothing outside the workspace.  The binding's signature table is checked against include/pdepth.h here too."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

import pdepth_amd
from pdepth_amd import _native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "probabilistic-depth_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# (B, V, C, D, H, W) -> byte offsets of (queue ints, packed source, statistics) and the total size.  Recorded from the
# library built at commit 3b67b78 (the last one with pdepth::sweep_ws_flag_only_bytes / sweep_ws_flag_bytes /
# sweep_ws_stats_offset / sweep_tiled_workspace_bytes, called through its visible C++ symbols).
PARENT_OFFSETS = {
    (4, 1, 67, 64, 256, 512): (32768, 33024, 171791616, 171799552),
    (2, 4, 67, 128, 512, 1024): (65536, 65792, 1358080256, 1358084352),
    (1, 2, 22, 48, 37, 53): (256, 512, 839936, 841984),
    (3, 1, 8, 16, 20, 31): (256, 512, 170496, 176640),
    (1, 1, 40, 64, 64, 128): (512, 768, 1724928, 1726976),
    (2, 2, 12, 16, 9, 35): (256, 512, 339712, 343808),     # ragged tiles, several items and views
    (2, 3, 5, 8, 4, 16): (256, 512, 57600, 61696),         # exactly one tile, C <= 8
    (1, 1, 76, 32, 8, 16): (256, 512, 43776, 45824),       # C > 72: only the channel-group-planar term sizes the packed region
}

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "sweep_workspace.hpp"

int main(int argc, char** argv) {   // B V C H W, five numbers per shape
    char* base = reinterpret_cast<char*>(uintptr_t(1) << 40);   // never dereferenced
    for (int i = 1; i + 4 < argc; i += 5) {
        pdepth::SweepArgs a{};
        a.B = atoi(argv[i]); a.V = atoi(argv[i + 1]); a.C = atoi(argv[i + 2]); a.H = atoi(argv[i + 3]); a.W = atoi(argv[i + 4]);
        const pdepth::SweepWorkspace ws = pdepth::SweepWorkspace::of(base, a);
        printf("%td %td %td %zu %td %d %td\n", reinterpret_cast<char*>(ws.queue) - base, ws.packed - base,
               reinterpret_cast<char*>(ws.stats) - base, pdepth::sweep_workspace_bytes(a.B, a.V, a.C, a.H, a.W),
               reinterpret_cast<char*>(ws.flags) - base, ws.nflags, reinterpret_cast<char*>(ws.dist_queue_counters()) - base);
    }
    return 0;
}
"""


def _desc(B, V, C, D, H, W, metric=_native.METRIC_L2):
    return _native.SweepDesc(B, V, C, D, H, W, metric, _native.ALGO_AUTO, _native.BLAS_FMA, 10.0, C * H * W, V * C * H * W, C * H * W)


def test_offsets_are_the_parent_builds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    shapes = list(PARENT_OFFSETS)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ws_offsets.hip"), os.path.join(tmp, "ws_offsets")
        open(src, "w").write(PROGRAM)
        r = subprocess.run([HIPCC, "-std=c++17", "--cuda-host-only", "-I", CSRC, src, "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        args = [str(n) for B, V, C, D, H, W in shapes for n in (B, V, C, H, W)]
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(shapes)
    lib = _native.load()
    for shape, row in zip(shapes, rows):
        queue, packed, stats, total = PARENT_OFFSETS[shape]
        assert row[:4] == (queue, packed, stats, total), (shape, row)
        # the tile flags start the workspace and end where the queue ints begin; the distance-form kernel's queue counters are
        # the tile-flag ints; the queue is 64 ints
        assert row[4:] == (0, queue // 4, 0) and packed - queue == 256, (shape, row)
        assert lib.pdepth_sweep_workspace_bytes(ctypes.byref(_desc(*shape))) == total, shape


def test_signature_table_covers_the_header():
    text = open(os.path.join(REPO, "include", "pdepth.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(pdepth_[a-z0-9_]+)\s*\(", text)))
    assert sorted(_native._SIGNATURES) == declared
    assert sorted(_native.EXPORTED_SYMBOLS) == declared
    lib = _native.load()
    for name, (restype, argtypes) in _native._SIGNATURES.items():
        fn = getattr(lib, name)
        assert restype is not None and fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name


@pytest.mark.gpu
@pytest.mark.parametrize("metric, tag, centred", [(_native.METRIC_L2, _native.LAYOUT_DIST16, True), (_native.METRIC_L1, _native.LAYOUT_C4, False)])
def test_regions_are_where_the_table_says_on_the_device(metric, tag, centred):
    import torch
    from pdepth_amd import synth
    shape = (2, 2, 12, 16, 9, 35)
    B, V, C, D, H, W = shape
    queue, packed, stats, total = PARENT_OFFSETS[shape]
    GUARD = 4096
    lib = _native.load()
    desc = _desc(*shape, metric=metric)
    assert lib.pdepth_sweep_source_layout(ctypes.byref(desc)) == tag
    assert lib.pdepth_sweep_workspace_bytes(ctypes.byref(desc)) == total
    dev = torch.device("cuda:0")
    b = synth.make_batch(41, B, C=C, D=D, H=H, W=W, V=V, pose="mono")
    d = {k: v.to(dev).contiguous() for k, v in b.items() if isinstance(v, torch.Tensor)}
    d_candi = torch.as_tensor(b["d_candi"], dtype=torch.float32).to(dev).contiguous()
    assert d_candi.numel() == D
    chan = torch.arange(1, C + 1, dtype=torch.float32, device=dev)
    src = chan.view(1, 1, C, 1, 1).expand(B, V, C, H, W).contiguous()   # channel c = c + 1 everywhere
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ws = buf.data_ptr() + GUARD
    cam = _native.Camera(d["K"].data_ptr(), d["R"].data_ptr(), d["t"].data_ptr(), d["rays"].data_ptr(), d["cxcy"].data_ptr())
    cost = torch.empty((B, D, H, W), dtype=torch.float32, device=dev)
    logp, depth = torch.empty_like(cost), torch.empty((B, H, W), dtype=torch.float32, device=dev)
    stream = _native._stream(dev)
    rc = lib.pdepth_pack_source_f32(ctypes.byref(desc), src.data_ptr(), ws, total, stream)
    assert rc == 0, lib.pdepth_last_error()
    rc = lib.pdepth_sweep_dpv_packed_f32(ctypes.byref(desc), ctypes.byref(cam), d["ref"].data_ptr(), d_candi.data_ptr(), cost.data_ptr(),
                                         logp.data_ptr(), depth.data_ptr(), ws, total, stream)
    assert rc == 0, lib.pdepth_last_error()
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == 0xA5).all()) and bool((host[GUARD + total:] == 0xA5).all())
    inner = host[GUARD: GUARD + total]
    at = queue + 4 * _native.LAYOUT_SLOT
    assert int(inner[at: at + 4].view(torch.int32).item()) == tag
    rows = inner[stats: stats + B * 496 * 4].view(torch.float32).view(B, 496)
    want = chan.cpu() if centred else torch.zeros(C)
    for i in range(B):
        print("item", i, "mu[0:12] =", rows[i, :C].tolist())
        assert torch.allclose(rows[i, :C], want, rtol=1e-5, atol=0.0), (i, rows[i, :C].tolist())
