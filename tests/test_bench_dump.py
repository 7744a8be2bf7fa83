"""bench.py's plain run and --dump-outputs.  CPU suite: the dump of the log-DPV and depth stays float32 and under 64 MB,
whole where it fits, else a fixed pixel sample that depends on the shape only.  GPU suite: a plain run times exactly --steps
steps, writes the last step's outputs and carries none of what --full adds."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sizes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_of_a_small_volume_is_whole(tmp_path):
    bench = _bench()
    logp, depth = torch.randn(2, 8, 16, 32), torch.randn(2, 16, 32)
    bench.dump_outputs(str(tmp_path), logp, depth)
    assert sorted(os.listdir(tmp_path)) == ["depth.npy", "logp.npy"]
    lp, dp = np.load(tmp_path / "logp.npy"), np.load(tmp_path / "depth.npy")
    assert lp.dtype == np.float32 and dp.dtype == np.float32
    assert np.array_equal(lp, logp.numpy()) and np.array_equal(dp, depth.numpy())


@pytest.mark.parametrize("shape", [(4, 64, 256, 512), (2, 128, 512, 1024)])
def test_dump_of_the_bench_volumes_is_a_fixed_sample_under_64_mb(tmp_path, shape):
    bench = _bench()
    B, D, H, W = shape
    g = torch.Generator().manual_seed(3)
    logp, depth = torch.randn(B, D, H, W, generator=g), torch.randn(B, H, W, generator=g)
    logp[0, 0] = torch.arange(H * W, dtype=torch.float32).view(H, W)   # plane 0 of item 0 names its pixels (exact in fp32)
    bench.dump_outputs(str(tmp_path / "a"), logp, depth)
    bench.dump_outputs(str(tmp_path / "b"), logp, depth)
    assert _sizes(tmp_path / "a") <= 64 << 20
    lp, dp = np.load(tmp_path / "a" / "logp.npy"), np.load(tmp_path / "a" / "depth.npy")
    assert lp.dtype == np.float32 and lp.shape[:2] == (B, D) and lp.ndim == 3 and lp.shape[2] < H * W
    assert np.array_equal(dp, depth.numpy())   # the depth map fits: whole
    # every plane at the same pixels: the sample is columns of the flattened maps, the same in every item
    flat = logp.reshape(B, D, H * W).numpy()
    cols = lp[0, 0].astype(np.int64)
    assert (np.diff(cols) > 0).all() and np.array_equal(flat[:, :, cols], lp)
    assert np.array_equal(lp, np.load(tmp_path / "b" / "logp.npy"))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_run_times_the_steps_and_dumps_them(tmp_path):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["higher_is_better"] is True and line["unit"] == "depth-volumes/s" and line["dtype"].startswith("f32")
    for key in ("cpu_baseline", "cold_start", "preflight", "model_real", "peaked", "packed_entry", "workloads"):
        assert key not in line, key
    lp, dp = np.load(out / "logp.npy"), np.load(out / "depth.npy")
    assert dp.shape == (4, 256, 512) and lp.shape[:2] == (4, 64) and _sizes(out) <= 64 << 20
