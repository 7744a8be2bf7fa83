"""Inputs of the loss fixture (tests/golden/g24_loss.npz), built the same way by the generator (which runs the reference on
them) and by the tests: numpy's frozen RandomState streams, float64 arithmetic rounded once to float32.  The fixture stores a
float64 checksum of every input, so a drift of these streams shows as a failed check, not as a wrong loss."""
import numpy as np
import torch

D, B = 16, 2
LO, HI = (9, 12), (36, 48)
VARIANCE = 0.3
MULS = {"ce_mul": 1.0, "dsc_mul": 1.0, "rsc_mul": 1.0, "smooth_mul": 0.5, "dc_mul": 0.25, "rsc_low_mul": 0.0}   # default_mono.json
SIDES = ("left", "right")


def d_candi():
    return [5.0 + (40.0 - 5.0) * v for v in np.linspace(0, 1, D)]   # powerf(5, 40, 16, 1)


def _log_dpv(rs, hw, scale):
    x = rs.randn(B, D, *hw) * scale
    x = x - x.max(1, keepdims=True)
    return (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)


def make_inputs():
    """-> dict of float32 arrays: for each side s and resolution r in (lo, hi): logp_s_r [B,D,h,w], dmap_s_r [B,h,w] (inside the
    candidate range, except a few pixels of dmap_right_lo / dmap_right_hi 20 m beyond it, masked out), mask_s_r [B,1,h,w];
    rgb_s [B,1,3,H,W]; K_lo, K_hi [B,3,3]; T_left2right [4,4].  mask_left_lo[1] has no entry equal to one (0.5 where valid: the
    cross-entropy of that item is 0 and it still weighs the consistency terms); mask_right_hi[0] holds one 0.5."""
    rs = np.random.RandomState(2400)
    out = {}
    for s in SIDES:
        for r, hw in (("lo", LO), ("hi", HI)):
            out[f"logp_{s}_{r}"] = _log_dpv(rs, hw, 2.0)
            dm = 5.5 + 34.0 * rs.rand(B, *hw)
            mk = (rs.rand(B, 1, *hw) < 0.7).astype(np.float64)
            if s == "right":   # out of range by 20 m: every Gaussian underflows, the label is -1 there; masked out
                dm[0, 1, 2:5] = 60.0
                mk[0, 0, 1, 2:5] = 0.0
            out[f"dmap_{s}_{r}"] = dm.astype(np.float32)
            out[f"mask_{s}_{r}"] = mk.astype(np.float32)
        base = rs.randn(B, 1, 3, HI[0] // 4 + 1, HI[1] // 4 + 1)
        up = np.kron(base, np.ones((4, 4)))[..., :HI[0], :HI[1]]
        out[f"rgb_{s}"] = (up + 0.1 * rs.randn(B, 1, 3, *HI)).astype(np.float32)
    out["mask_left_lo"][1] *= 0.5
    out["mask_right_hi"][0, 0, 20, 30] = 0.5
    K = np.array([[41.0, 0.0, 24.3], [0.0, 40.0, 17.6], [0.0, 0.0, 1.0]])
    Kl = K.copy()
    Kl[:2] *= 0.25
    out["K_hi"] = np.tile(K, (B, 1, 1)).astype(np.float32)
    out["K_lo"] = np.tile(Kl, (B, 1, 1)).astype(np.float32)
    a = 0.01
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T[:3, 3] = [-0.54, 0.01, 0.02]
    out["T_left2right"] = T.astype(np.float32)
    return out


def checksums(inp):
    return {"sum_" + k: np.float64(v.astype(np.float64).sum()) for k, v in inp.items()}


def soft_labels(inp, gen, s, r):
    """List of [D,h,w] labels of side s at resolution r from the RAW depth maps: gen = gen_soft_label_torch of either side."""
    var = torch.tensor(VARIANCE)
    return [gen(d_candi(), torch.from_numpy(inp[f"dmap_{s}_{r}"][i]), var, zero_invalid=True) for i in range(B)]


def structure(inp, gen, dev="cpu", dtype=torch.float32, with_labels=True):
    """(output, target) of BaseLoss.forward; the four volumes are leaves that require grad."""
    def t(a):
        return torch.from_numpy(a).to(dtype).to(dev)
    output, target = [], []
    for s in SIDES:
        output.append({"output": [t(inp[f"logp_{s}_lo"]).requires_grad_(True)],
                       "output_refined": [t(inp[f"logp_{s}_hi"]).requires_grad_(True)]})
        tg = {"masks": t(inp[f"mask_{s}_lo"]), "masks_imgsizes": t(inp[f"mask_{s}_hi"]), "intrinsics": t(inp["K_lo"]),
              "intrinsics_up": t(inp["K_hi"]), "rgb": t(inp[f"rgb_{s}"]), "T_left2right": torch.from_numpy(inp["T_left2right"]).to(dtype),
              "d_candi": d_candi(), "dmaps": t(inp[f"dmap_{s}_lo"]), "dmap_imgsizes": t(inp[f"dmap_{s}_hi"])}
        if with_labels:
            tg["soft_labels"] = [l.to(dtype).to(dev) for l in soft_labels(inp, gen, s, "lo")]
            tg["soft_labels_imgsize"] = [l.to(dtype).to(dev) for l in soft_labels(inp, gen, s, "hi")]
        target.append(tg)
    return tuple(output), tuple(target)


def volumes(output):
    return [output[0]["output"][0], output[0]["output_refined"][0], output[1]["output"][0], output[1]["output_refined"][0]]


class Cfg:
    """cfg.loss.* / cfg.var.softce / cfg.data.loss_name, attribute style."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def loss_cfg():
    return Cfg(loss=Cfg(**MULS), var=Cfg(softce=VARIANCE), data=Cfg(loss_name="base"))
