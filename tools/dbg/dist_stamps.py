"""Phase stamps of the distance-form sweep kernel (library built with -DDIST_STAMPS): cycles per phase, per wave and pass.

    PDEPTH_LIB=<stamps library> python tools/dbg/dist_stamps.py [mono] [stereo]
        one library: the sum over the four waves of a workgroup (-DDIST_STAMP_WAVE=w: wave w alone)
    python tools/dbg/dist_stamps.py --libs <w0.so> <w1.so> <w2.so> <w3.so> -- [mono] [stereo]
        four libraries built with -DDIST_STAMP_WAVE=0 .. 3, each run in a child process of its own: the four waves side by
        side.  A wave whose barrier stamp (B1, B2, B3) is near zero is the one the other three waited for there."""
import json, os, subprocess, sys
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
NAMES = ["queue", "set-up+loads issued", "positions", "table+centring", "B1", "operands+scan", "slots+X", "wait Q", "B2", "combine", "stores+softmax", "B3+merge+stores"]


def measure(pose):
    """-> (stamp sums of the launch, passes of the launch)"""
    import torch
    import pdepth_amd  # noqa: F401
    from pdepth_amd import ops, synth, _native
    B, C, D, H, W, V = (int(x) for x in os.environ.get("STAMP_SHAPE", "4,67,64,256,512,1").split(","))
    b = synth.make_batch(2, B, C=C, D=D, H=H, W=W, V=V, pose=pose)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
    dc = ops.d_candi_tensor(d["d_candi"], "cuda")
    for _ in range(3):
        ops.sweep_dpv(d["ref"], d["src"], d["K"], d["R"], d["t"], d["rays"], d["cxcy"], dc, 10.0, algo="dist")
    torch.cuda.synchronize()
    ws = _native._last_workspace
    n = B * ((W + 15) // 16) * ((H + 3) // 4)
    flag_only = (4 * n + 255) & ~255
    acc = ws[flag_only + 32: flag_only + 32 + 96].view(torch.int64).cpu().tolist()
    return acc, B * H * W // 16 * V


def main(argv):
    if argv[:1] == ["--json"]:   # (child of --libs)
        print("STAMPS " + json.dumps({pose: measure(pose) for pose in argv[1:]}))
        return
    if argv[:1] == ["--libs"]:
        libs, poses = argv[1:5], [a for a in argv[5:] if a != "--"] or ["mono", "stereo"]
        cols = []
        for lib in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--json"] + poses, env=dict(os.environ, PDEPTH_LIB=lib),
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("%s: exit status %d\n%s" % (lib, r.returncode, r.stderr[-2000:]))
            cols.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("STAMPS ")][-1][7:]))
        for pose in poses:
            passes = cols[0][pose][1]
            print("%s: cycles per pass, wave 0 .. 3 of a workgroup (%d passes)" % (pose, passes))
            for i, nm in enumerate(NAMES):
                print("   %-22s" % nm + "".join(" %8.0f" % (c[pose][0][i] / passes) for c in cols))
            print("   %-22s" % "whole pass" + "".join(" %8.0f" % (sum(c[pose][0]) / passes) for c in cols))
        return
    for pose in argv or ["mono", "stereo"]:
        acc, passes = measure(pose)
        tot = sum(acc)
        print("%s: cycles per wave and pass (4 waves x %d passes), total %.0f" % (pose, passes, tot / (4 * passes)))
        for nm, a in zip(NAMES, acc):
            print("   %-22s %8.0f  %5.1f %%" % (nm, a / (4 * passes), 100.0 * a / tot))


if __name__ == "__main__":
    main(sys.argv[1:])
