"""Round 4: (1) the HIP ops of EVERY feedback step of a five-frame window on the reference's own tensors (fixture g22,
tests/golden/make_golden_r4.py) -- teacher forcing: what is asserted per frame is the op, not the 3-D network in front of
it; (2) the RCCL code path of dist.py / bench.py, once, on the hardware.

  warp_feature                      models/models.py:616-625     1e-5 abs (bit-faithful positions, bilinear taps)
  log_softmax(BV_cur + BV_resi)     models/models.py:694         2e-5 abs on the log-DPV, 1e-4 m on E[d]
  the decoder's log_softmax + E[d]  models/models.py:351, trainer/default_trainer.py:230-233   the same bounds
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import harness, ops, synth
from oracle import ref_cpu as O
from util import golden, golden_blas

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGP_ATOL, DEPTH_ATOL = 2e-5, 1e-4


def _frames(g):
    hw = [int(v) for v in g["image_hw"]]
    for frame in range(1, int(g["nframes"])):
        yield frame, "f%d_" % frame, synth.make_model_input(int(g["input_seed0"]) + frame, B=1, V=1, H=hw[0], W=hw[1], D=64, pose="mono")


def test_oracle_reproduces_every_feedback_step_of_the_window():
    g = golden("g22_feedback_window.npz")
    for frame, f, inp in _frames(g):
        upd = torch.log_softmax(torch.from_numpy(g[f + "BV_cur"]) + torch.from_numpy(g[f + "BV_resi"]), dim=1)
        np.testing.assert_allclose(upd.numpy()[:, ::2], g[f + "BV_upd_even"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(O.dpv_to_depthmap(upd, inp["d_candi"], BV_log=True).numpy(), g[f + "depth_low"], rtol=0, atol=2e-5)
        dec = torch.log_softmax(torch.from_numpy(g[f + "dec_pre_crop"]), dim=1)
        np.testing.assert_allclose(dec.numpy()[:, ::2], g[f + "dec_logp_even"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(O.dpv_to_depthmap(dec, inp["d_candi"], BV_log=True).numpy(), g[f + "depth_ref_crop"], rtol=0, atol=2e-5)


@pytest.mark.gpu
def test_hip_feedback_ops_on_the_reference_tensors_of_every_frame():
    """Frames 1-4 of the window: the feedback update (reduce_ex with addend), the decoder's DPV pass and warp_feature, each on
    the tensors the reference had at that point of that frame; depth within 1e-4 m per frame."""
    g = golden("g22_feedback_window.npz")
    r0, r1 = [int(v) for v in g["rows"]]
    worst = {"upd_logp": 0.0, "upd_depth": 0.0, "dec_logp": 0.0, "dec_depth": 0.0, "warp": 0.0}
    for frame, f, inp in _frames(g):
        cur, resi = torch.from_numpy(g[f + "BV_cur"]).to(DEV), torch.from_numpy(g[f + "BV_resi"]).to(DEV)
        r = ops.dpv_reduce_ex(cur, inp["d_candi"], addend=resi, want_logp=True, want_prob=True, want_depth=True)
        el = np.abs(r["logp"].cpu().numpy()[:, ::2] - g[f + "BV_upd_even"]).max()
        ed = np.abs(r["depth"].cpu().numpy() - g[f + "depth_low"]).max()
        assert el <= LOGP_ATOL and ed <= DEPTH_ATOL, f"frame {frame}: feedback update differs by {el:.2e} (log-DPV), {ed:.2e} m"
        np.testing.assert_allclose(r["prob"].cpu().numpy()[:, ::2], np.exp(g[f + "BV_upd_even"]), rtol=2e-5, atol=1e-7)
        pre = torch.from_numpy(g[f + "dec_pre_crop"]).to(DEV).contiguous()
        logp, depth = ops.dpv_reduce(pre, inp["d_candi"])
        dl = np.abs(logp.cpu().numpy()[:, ::2] - g[f + "dec_logp_even"]).max()
        dd = np.abs(depth.cpu().numpy() - g[f + "depth_ref_crop"]).max()
        assert dl <= LOGP_ATOL and dd <= DEPTH_ATOL, f"frame {frame}: decoder DPV pass differs by {dl:.2e} (log-DPV), {dd:.2e} m"
        # warp_feature on every 4th channel with every 4th plane: channel i only ever meets plane i
        feat = torch.from_numpy(g[f + "feat_raw_c4"]).to(DEV)            # [1, V+1, 16, h, w]
        poses, K = inp["src_cam_poses"].to(DEV), inp["intrinsics"].to(DEV)
        out = ops.warp_feature(feat, K, poses[:, :, :3, :3].contiguous(), poses[:, :, :3, 3].contiguous(), inp["unit_ray"].to(DEV),
                               K[:, :2, 2].contiguous(), inp["d_candi"][::4], blas=golden_blas(g))
        ew = np.abs(out.cpu().numpy()[:, :, :, r0:r1] - g[f + "warped_c4"]).max()
        scale = float(np.abs(g[f + "warped_c4"]).max())
        assert ew <= 1e-5 * max(1.0, scale), f"frame {frame}: warp_feature differs by {ew:.2e} (values up to {scale:.2f})"
        for k, v in (("upd_logp", el), ("upd_depth", ed), ("dec_logp", dl), ("dec_depth", dd), ("warp", ew)):
            worst[k] = max(worst[k], float(v))
    print("feedback window on reference tensors, worst over frames 1-4:", json.dumps(worst))


_RCCL_CHILD = r"""
import json, os, sys, time
sys.path.insert(0, {repo!r})
import torch
import pdepth_amd
from pdepth_amd import dist as pdist
rank, world, local_rank = pdist.init_from_env()
assert (rank, world, local_rank) == (0, 1, 0), (rank, world, local_rank)
assert torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl", torch.distributed.get_backend()
dev = torch.device("cuda", local_rank)
torch.cuda.set_device(dev)
m = torch.tensor([4.0, 0.5, 17.25, 1.0], dtype=torch.float32, device=dev)
allm = pdist.gather_metrics(m).cpu()
assert tuple(allm.shape) == (1, 4) and torch.equal(allm[0], m.cpu())
pdist.barrier()
assert pdist.max_over_ranks(1.25, dev) == 1.25
lo, hi = pdist.shard_range(4, rank, world)
assert (lo, hi) == (0, 4)
torch.distributed.destroy_process_group()
print(json.dumps({{"backend": "nccl", "world": world, "ok": True}}))
"""


@pytest.mark.gpu
def test_rccl_path_initialises_on_the_hardware():
    """dist.py with backend nccl (= RCCL) in a fresh child process, WORLD_SIZE = 1: init_from_env, the all_gather of the metric
    vector, the MAX all-reduce and the barrier -- the calls bench.py makes at N > 1 -- and then bench.py itself under
    torch.distributed.run.  The children are started from a parent that may have touched the GPU: they are new processes
    (subprocess, no exec of this one)."""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29731",
               HSA_ENABLE_IPC_MODE_LEGACY="0", PDEPTH_DIST_FORCE="1")
    p = subprocess.run([sys.executable, "-c", _RCCL_CHILD.format(repo=REPO)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["ok"] is True
    env2 = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env2["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env2["PDEPTH_DIST_FORCE"] = "1"   # (a single rank would not open a process group otherwise)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29733", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-cold"], env=env2, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["value"] > 0 and line["scaling"] == "weak"
    # SURVEY section 8(d) "Ambiguity resolved": the 64x128 model-real figure and the peaked variant ride in the driver's line
    # (VERDICT r4, item 4): B = 1 and B = 4, both entries, with us per call, launches per call and the roofline fraction
    assert line["roofline"]["sweep_kernel"] == "dist" and line["packed_entry"]["max_abs_depth_diff_vs_headline"] <= 1e-4
    for key in ("B1_nchw", "B1_packed", "B4_nchw", "B4_packed"):
        row = line["model_real"][key]
        assert row["us_per_call"] > 0 and row["launches"] >= 1 and 0 < row["frac"] < 1 and row["volumes_per_s"] > 0, key
    assert line["model_real"]["B1_packed"]["launches"] == 1 and "64x128" in line["model_real"]["shape"]
    assert line["peaked"]["ms_per_step"] > 0 and line["peaked"]["value"] > 0


@pytest.mark.gpu
def test_packnet_model_with_a_plugged_in_network():
    """get_model('packnet') (models/get_model.py:9-10, models/packnet.py:304-406): with a stand-in for the PackNet CNN
    (a strided convolution as base_encoder, an interpolation as base_decoder) the host object returns the reference's
    dictionary, its log-DPV is the oracle's sweep -> log_softmax chain on the encoder's own feature maps (:362-394) and the
    feature_set has the reference's [view][level] layout."""
    from pdepth_amd.models import get_model
    from util import oracle_batch

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = torch.nn.Conv2d(3, 8, 3, stride=2, padding=1)
            self.c2 = torch.nn.Conv2d(8, 13, 3, stride=2, padding=1)

        def forward(self, rgb):
            a = torch.relu(self.c1(rgb))
            b = self.c2(a)
            return [a, b], b

    class Dec(torch.nn.Module):
        def forward(self, dpv, feats):
            assert len(feats) == 2 and feats[1].shape[1] == 13
            return torch.log_softmax(torch.nn.functional.interpolate(torch.log(dpv.clamp_min(1e-30)), scale_factor=2.0), dim=1)

    torch.manual_seed(3)
    cfg = synth.default_cfg("default")
    cfg.data["model_name"] = "packnet"
    model = get_model(cfg, 0).attach_networks(Enc(), Dec()).to(DEV).eval()
    inp = harness.move_input(synth.make_model_input(11, B=2, V=2, H=96, W=160, D=48, pose="mono"), DEV)
    out = model(inp)
    assert set(out) == {"output", "output_refined", "flow", "flow_refined"} and out["flow"] is None
    BV = out["output"][0]
    assert BV.shape == (2, 48, 24, 40) and out["output_refined"][0].shape == (2, 48, 48, 80)
    # the reference's chain on the same feature maps, on the CPU
    with torch.no_grad():
        rgb = inp["rgb"]
        flat = rgb.reshape(-1, 3, 96, 160)
        feat = model.base_encoder(flat)[1]
        both = torch.cat((feat, torch.nn.functional.avg_pool2d(flat, 4)), dim=1).view(2, 3, 16, 24, 40).cpu()
    poses = inp["src_cam_poses"].cpu()
    K = inp["intrinsics"].cpu()
    b = {"ref": both[:, -1], "src": both[:, :-1], "K": K, "R": poses[:, :-1, :3, :3], "t": poses[:, :-1, :3, 3],
         "rays": inp["unit_ray"].cpu(), "cxcy": K[:, :2, 2].contiguous(), "d_candi": inp["d_candi"]}
    _, ologp, _ = oracle_batch(b, sigma=cfg.var.sigma_soft_max)
    np.testing.assert_allclose(BV.cpu().numpy(), ologp.numpy(), rtol=0, atol=5e-5)
    BV2, feature_set = model.forward_encoder(inp)
    assert torch.equal(BV2, BV) and len(feature_set) == 3 and [tuple(t.shape) for t in feature_set[-1]] == [(2, 8, 48, 80), (2, 13, 24, 40)]


@pytest.mark.gpu
def test_packed_entry_is_one_capturable_launch():
    """the per-item call of models/models.py:528-550 as the host model issues it -- a sweep on an already
    packed source -- is ONE kernel launch with no host synchronisation, no allocation and no clearing launch in front: it
    can be captured into a hipGraph (torch.cuda.CUDAGraph on ROCm) and replayed on new reference features, camera poses and
    an unchanged workspace, with the results of the eager call bit for bit."""
    b = synth.make_batch(5, 1, C=67, D=64, H=64, W=128, V=1, pose="mono")
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    dc = ops.d_candi_tensor(d["d_candi"], DEV)
    ps = ops.pack_source(d["src"], 64)
    ref, R, t = d["ref"].clone(), d["R"].clone(), d["t"].clone()
    run = lambda: ops.sweep_dpv(ref, ps, d["K"], R, t, d["rays"], d["cxcy"], dc, 10.0)
    want0 = [x.clone() for x in run()[1:]]           # (also warms the per-device caches of the launcher: not capturable work)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[1], want0[0]) and torch.equal(out[2], want0[1])
    # new inputs in the captured buffers: another frame's reference features and pose
    b2 = synth.make_batch(6, 1, C=67, D=64, H=64, W=128, V=1, pose="mono")
    ref.copy_(b2["ref"].to(DEV)); R.copy_(b2["R"].to(DEV)); t.copy_(b2["t"].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = [out[1].clone(), out[2].clone()]
    want = run()
    assert torch.equal(got[0], want[1]) and torch.equal(got[1], want[2])
    import time
    t0 = time.perf_counter()
    for _ in range(200):
        graph.replay()
    torch.cuda.synchronize()
    print("graph replay of the packed-entry sweep, B=1 64x128: %.1f us per call (wall, back to back)" % ((time.perf_counter() - t0) / 200 * 1e6))


@pytest.mark.gpu
def test_image_sizes_that_are_not_a_multiple_of_the_map(monkeypatch):
    """an image of (4 h + r) x (4 w + r') pixels -- F.avg_pool2d drops the remainder rows / columns -- is refused
    by the encoder epilogue (ops.UnsupportedShape, not wrong strides), the head falls back to cat + avg_pool2d + the packed
    sweep and gives what that chain gives; and a native failure that is NOT about the shape is not swallowed."""
    from pdepth_amd import _native
    from pdepth_amd.models.packnet_head import PacknetHead
    torch.manual_seed(1)
    enc = torch.nn.Conv2d(3, 9, 7, stride=4, padding=3).to(DEV)
    feat = torch.randn(4, 9, 16, 24, device=DEV)
    with pytest.raises(ops.UnsupportedShape):
        ops.pack_views(feat, torch.randn(4, 3, 66, 96, device=DEV), 2, 32)      # 66 = 4 * 16 + 2 rows
    with pytest.raises(ops.UnsupportedShape):
        ops.pack_views(feat, torch.randn(4, 3, 64, 99, device=DEV), 2, 32)      # 99 = 4 * 24 + 3 columns
    inp = harness.move_input(synth.make_model_input(21, B=2, V=1, H=64, W=96, D=32, pose="mono"), DEV)
    calls = [0]

    def counted(x):
        calls[0] += 1
        return enc(x)[:, :, :16, :24]
    head = PacknetHead(synth.default_cfg("default"), encoder=counted)
    BV0, depth0 = head(inp)                                                                          # exact multiple: the epilogue kernel
    rgb = torch.nn.functional.pad(inp["rgb"], (0, 3, 0, 2))                                         # 66 x 99: the same pooled image
    BV1, depth1 = head(dict(inp, rgb=rgb))
    assert calls[0] == 2, "the fallback must reuse the encoder's output (ADVICE r4), not run the encoder again"
    # (the encoder sees the padded frame: compare against the chain the reference runs on that frame)
    with torch.no_grad():
        flat = rgb.reshape(-1, 3, 66, 99)
        f = enc(flat)[:, :, :16, :24]
        both = torch.cat((f, torch.nn.functional.avg_pool2d(flat, 4)), dim=1).view(2, 2, 12, 16, 24)
    poses, K = inp["src_cam_poses"].float(), inp["intrinsics"].float()
    _, BVr, depthr = ops.sweep_dpv(both[:, -1], both[:, :-1], K, poses[:, :-1, :3, :3], poses[:, :-1, :3, 3], inp["unit_ray"].float(),
                                   K[:, :2, 2].contiguous(), inp["d_candi"], head.sigma_soft_max)
    # (the fallback packs the source views without the reference view's statistics, the NCHW entry sees both: equal to rounding)
    assert torch.allclose(BV1, BVr, rtol=0, atol=1e-4) and torch.allclose(depth1, depthr, rtol=0, atol=1e-4)
    assert BV0.shape == BV1.shape
    # a native failure that has nothing to do with the shape propagates (it is not turned into the fallback)
    def broken(*a, **k):
        raise RuntimeError("pdepth_pack_views_f32: launch failed (injected)")
    monkeypatch.setattr(ops, "pack_views", broken)
    with pytest.raises(RuntimeError, match="injected"):
        head(inp)


def test_bench_line_declares_what_ran_before_the_timed_steps():
    """ADVICE r3 / VERDICT r3 weak 7: the committed bench line of this round says what GPU work preceded the headline's
    warm-up (preheat_ms, the cold-start figure with exactly --warmup steps as the first work of the process) and where
    and when its PMC traffic record was collected."""
    line = json.loads(open(os.path.join(REPO, "profiles", "r04_bench_line.json")).read().strip().splitlines()[-1])
    assert line["cold_start"]["ms_per_step"] > 0 and "first GPU work" in line["cold_start"]["what"]
    assert line["preheat_ms"] > 0 and "cold_start" in line["preheat"]
    assert line["roofline"]["traffic_collected"] and line["roofline"]["traffic"] > line["roofline"]["achieved"] * 0   # present
    assert line["roofline"]["sweep_kernel"] == "corr" and line["packed_entry"]["max_abs_depth_diff_vs_headline"] == 0.0
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["max_abs_depth_diff_gpu_vs_port_item0"] <= 1e-4
