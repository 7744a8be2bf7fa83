"""Host model with the reference's module contract, hot path on the HIP kernels.

Stands in for the reference's models/models.py: same constructor arguments
(``cfg.var.{sigma_soft_max, feature_dim, nmode, ndepth, bn_avg}``), same ``forward(inputs: list[dict])
-> list[dict]`` with keys ``output / output_refined / flow / flow_refined`` (models.py:706-710, :656),
``init_weights()``, ``set_viz()``, and the same parameter names in the same registration order, so a
reference checkpoint loads by name and by the trainer's positional zip (trainer/base_trainer.py:83-90).

What is different -- on purpose:
  * the plane sweep is ONE batched launch of the HIP kernel (ops.sweep_cost) on views of the encoder
    output, replacing the per-item Python loop with its per-item D2H copy of the intrinsics
    (models.py:528-550, :538);
  * warp_feature is the diagonal kernel (1/D of the reference's work), batched;
  * every log_softmax over the depth axis goes through ops.dpv_reduce;
  * Base3D registers its residual blocks (the reference keeps them in a plain Python list, so their
    110 848 parameters are missing from its state_dict and pinned to .cuda(id), models.py:394-399).
    They are registered LAST, so positional loading of a reference checkpoint is unaffected.
The convolution stacks are stock torch.nn (MIOpen on ROCm); they are not part of the hot path.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

EPSILON = torch.finfo(float).eps  # reference: utils/img_utils.py:12


# ------------------------------------------------------------------------------------------------
# building blocks (attribute names and Sequential nesting fix the state_dict keys)
# ------------------------------------------------------------------------------------------------
def _conv_bn(cin, cout, k, stride, pad, dilation, track):
    return nn.Sequential(
        nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=dilation if dilation > 1 else pad,
                  dilation=dilation, bias=False),
        nn.BatchNorm2d(cout, track_running_stats=track))


def _conv_bn_3d(cin, cout, track):
    return nn.Sequential(nn.Conv3d(cin, cout, kernel_size=3, padding=1, stride=1, bias=False),
                         nn.BatchNorm3d(cout, track_running_stats=track))


def _conv_lrelu(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=True), nn.LeakyReLU())


def _deconv_lrelu(cin, cout):
    return nn.Sequential(nn.ConvTranspose2d(cin, cout, kernel_size=4, stride=2, padding=1, bias=True),
                         nn.LeakyReLU())


def _he_init(m):
    """normal(0, sqrt(2/n)) convs, unit BN, bilinear transposed convs (reference models.py:226-240,:353-374)."""
    if isinstance(m, (nn.Conv2d, nn.Conv3d)):
        n = m.out_channels
        for k in m.kernel_size:
            n *= k
        m.weight.data.normal_(0, math.sqrt(2.0 / n))
    elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
        m.weight.data.fill_(1)
        m.bias.data.zero_()
    elif isinstance(m, nn.Linear):
        m.bias.data.zero_()
    elif isinstance(m, nn.ConvTranspose2d):
        n = m.kernel_size[1]
        factor = (n + 1) // 2
        center = factor - 1 if n % 2 == 1 else factor - 0.5
        og = np.ogrid[:n, :n]
        w = (1 - abs(og[0] - center) / factor) * (1 - abs(og[1] - center) / factor)
        m.weight.data.copy_(torch.from_numpy(w))


class _Residual(nn.Module):
    """conv-bn-relu, conv-bn, (+ 1x1 projection) -- PSMNet basic block."""

    def __init__(self, cin, cout, stride, downsample, pad, dilation, track):
        super().__init__()
        self.conv1 = nn.Sequential(_conv_bn(cin, cout, 3, stride, pad, dilation, track), nn.ReLU(inplace=True))
        self.conv2 = _conv_bn(cout, cout, 3, 1, pad, dilation, track)
        self.downsample = downsample

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        return y + (x if self.downsample is None else self.downsample(x))


class BaseEncoder(nn.Module):
    """PSMNet-style feature pyramid: returns (1/2-res features, raw 1/4-res features, 1/4-res features)."""

    def __init__(self, feature_dim=32, bn_running_avg=False, multi_scale=True):
        super().__init__()
        mul = feature_dim / 64.0
        s0, s1, s2, s3 = int(16 * mul), int(32 * mul), int(64 * mul), int(128 * mul)
        self.multi_scale = multi_scale
        self._track = bn_running_avg
        self._cin = s1
        t = bn_running_avg
        self.firstconv = nn.Sequential(_conv_bn(3, s1, 3, 2, 1, 1, t), nn.ReLU(inplace=True),
                                       _conv_bn(s1, s1, 3, 1, 1, 1, t), nn.ReLU(inplace=True),
                                       _conv_bn(s1, s1, 3, 1, 1, 1, t), nn.ReLU(inplace=True))
        self.layer1 = self._stage(s1, 3, 1, 1, 1)
        self.layer2 = self._stage(s2, s0, 2, 1, 1)
        self.layer3 = self._stage(s3, 3, 1, 1, 1)
        self.layer4 = self._stage(s3, 3, 1, 1, 2)
        for i, k in enumerate((64, 32, 16, 8), start=1):
            setattr(self, "branch%d" % i, nn.Sequential(nn.AvgPool2d((k, k), stride=(k, k)),
                                                        _conv_bn(s3, s1, 1, 1, 0, 1, t), nn.ReLU(inplace=True)))
        self.lastconv = nn.Sequential(_conv_bn(s1 * 4 + s2 + s3, s3, 3, 1, 1, 1, t), nn.ReLU(inplace=True),
                                      nn.Conv2d(s3, feature_dim, kernel_size=1, padding=0, stride=1, bias=False))
        self.apply(_he_init)

    def _stage(self, cout, blocks, stride, pad, dilation):
        proj = None
        if stride != 1 or self._cin != cout:
            proj = nn.Sequential(nn.Conv2d(self._cin, cout, kernel_size=1, stride=stride, bias=False),
                                 nn.BatchNorm2d(cout, track_running_stats=self._track))
        units = [_Residual(self._cin, cout, stride, proj, pad, dilation, self._track)]
        self._cin = cout
        units += [_Residual(cout, cout, 1, None, pad, dilation, self._track) for _ in range(1, blocks)]
        return nn.Sequential(*units)

    def forward(self, x):
        half = self.layer1(self.firstconv(x))
        raw = self.layer2(half)
        skip = self.layer4(self.layer3(raw))
        size = (skip.shape[2], skip.shape[3])
        pooled = [F.interpolate(getattr(self, "branch%d" % i)(skip), size, mode="bilinear", align_corners=True)
                  for i in (4, 3, 2, 1)]
        feat = self.lastconv(torch.cat([raw, skip] + pooled, 1))
        return (half, raw, feat) if self.multi_scale else feat


class BaseDecoder(nn.Module):
    """DPV (D as channels) + image features at 1/4, 1/2, 1 resolution -> full-resolution log-DPV."""

    def __init__(self, C0, C1, C2, D=64, upsample_D=False):
        super().__init__()
        d0 = 2 * D if upsample_D else D
        d1 = 2 * d0 if upsample_D else D
        cin = D + C0
        self.conv0 = _conv_lrelu(cin, cin)
        self.conv0_1 = _conv_lrelu(cin, cin)
        self.trans_conv0 = _deconv_lrelu(cin, d0)
        self.conv1 = _conv_lrelu(d0 + C1, d0 + C1)
        self.conv1_1 = _conv_lrelu(d0 + C1, d0 + C1)
        self.trans_conv1 = _deconv_lrelu(d0 + C1, d1)
        self.conv2 = _conv_lrelu(d1 + C2, d1 + C2)
        self.conv2_1 = _conv_lrelu(d1 + C2, d1)
        self.conv2_2 = nn.Conv2d(d1, d1, kernel_size=3, stride=1, padding=1, bias=True)
        self.apply(_he_init)

    def forward(self, dpv_raw, img_features, d_candi=None):
        """Returns the refined log-DPV.  With d_candi, the same pass over the full-resolution volume also leaves the
        refined depth map and the nearest quarter-resolution log-DPV (the next frame's prev_output,
        trainer/default_trainer.py:221) in self.aux for the evaluation harness."""
        x = self.conv0_1(self.conv0(torch.cat([dpv_raw, img_features[0]], dim=1)))
        x = self.conv1_1(self.conv1(torch.cat([self.trans_conv0(x), img_features[1]], dim=1)))
        x = self.conv2_2(self.conv2_1(self.conv2(torch.cat([self.trans_conv1(x), img_features[2]], dim=1))))
        self.aux = None
        if d_candi is not None and x.shape[2] >= 4 and x.shape[3] >= 4:
            r = ops.dpv_reduce_ex(x, d_candi, want_logp=True, want_depth=True, want_quarter=True, inplace=True)  # models.py:351
            self.aux = {"depth_refined": r["depth"], "prev_output": r["quarter"]}
            return r["logp"]
        logp, _ = ops.dpv_reduce(x, None, want_logp=True, want_depth=False, inplace=True)  # models.py:351
        return logp


class Base3D(nn.Module):
    """3-D residual CNN over [B, 4, D, h, w] (feedback mode)."""

    def __init__(self, input_volume_channels, feature_dim=32, dres_count=4, bn_running_avg=False, id=0):
        super().__init__()
        t = bn_running_avg
        self.dres0 = nn.Sequential(_conv_bn_3d(input_volume_channels, feature_dim, t), nn.ReLU(),
                                   _conv_bn_3d(feature_dim, feature_dim, t), nn.ReLU())
        self.classify = nn.Sequential(_conv_bn_3d(feature_dim, feature_dim, t), nn.ReLU(),
                                      nn.Conv3d(feature_dim, 1, kernel_size=3, padding=1, stride=1, bias=False))
        # registered (unlike the reference) and registered last -- see the module docstring
        self.dres_modules = nn.ModuleList(
            nn.Sequential(_conv_bn_3d(feature_dim, feature_dim, t), nn.ReLU(), _conv_bn_3d(feature_dim, feature_dim, t))
            for _ in range(dres_count))
        self.apply(_he_init)
        # The reference's residual blocks sit in a plain list, so model.eval() never reaches them and
        # their BatchNorm3d layers normalise with BATCH statistics even at evaluation time
        # (models.py:394-399 + trainer/default_trainer.py:180).  Reproduced by default so outputs match;
        # set to False for conventional eval-mode BatchNorm.
        self.reference_bn_quirk = True

    def train(self, mode=True):
        super().train(mode)
        if self.reference_bn_quirk:
            self.dres_modules.train(True)
        return self

    def forward(self, input_volume, prob=True):
        cost = self.dres0(input_volume.contiguous())
        for block in self.dres_modules:
            cost = block(cost) + cost
        res = self.classify(cost).squeeze(1)
        if prob:
            res, _ = ops.dpv_reduce(res.contiguous(), None, want_logp=True, want_depth=False, inplace=True)
        return res


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
def _tolerate_missing_dres_blocks(module, incompatible_keys):
    """A reference checkpoint has NO key of Base3D's residual blocks (they live in a plain list there, models.py:394-399):
    then, and only then, their absence is not an error.  A checkpoint that holds some of them but not all is truncated."""
    def is_dres(k):
        return ".dres_modules." in k or k.startswith("dres_modules.")
    # (torch fills a missing BatchNorm num_batches_tracked itself and does not report it)
    expected = {k for k in module.state_dict().keys() if is_dres(k) and not k.endswith("num_batches_tracked")}
    missing = {k for k in incompatible_keys.missing_keys if is_dres(k)}
    if expected and missing >= expected:
        incompatible_keys.missing_keys[:] = [k for k in incompatible_keys.missing_keys if not is_dres(k)]


class _SweepFeatures:
    """What BaseModel._features hands to the sweep on the default path: the source views in the kernels' staging layout, the
    reference view as NCHW -- both with the pooled image appended -- and the encoder's learned feature maps, which is all
    that the callers' slices `feats[:, v, :-3]` (decoder skip connections, models.py:563-564) ever read."""

    def __init__(self, learned, packed, ref):
        self.learned, self.packed, self.ref = learned, packed, ref   # [B,V1,Cf,h,w], PackedSource, [B,Cf+3,h,w]

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 3 and idx[2] == slice(None, -3, None):
            return self.learned[idx[0], idx[1]]
        raise IndexError("only feats[:, v, :-3] (the learned channels of one view) can be read from the packed features")


class BaseModel(nn.Module):
    """Host model.  All three nmodes -- "default", "default_upsample" and "default_feedback" -- train: with grad mode on, the
    sweep, the DPV reductions, the DPV fusion and the feedback path's warp_feature run through their HIP backward passes (ops:
    gradients with respect to the feature maps and the volumes; the sweep then takes the concatenated NCHW features; the
    sparse depth maps and masks of the fusion are data), so forward + loss.backward() work as in the reference's training loop
    (trainer/default_trainer.py:87-169).  In "default_feedback" the caller detaches prev_output between frames, as that loop
    does (trainer/default_trainer.py:144-146).  sweep_deterministic selects the bit-reproducible sums of the sweep's and the
    warp's scattered gradients."""

    def __init__(self, cfg, id):
        super().__init__()
        self.cfg = cfg
        self.sigma_soft_max = self.cfg.var.sigma_soft_max
        self.feature_dim = self.cfg.var.feature_dim
        self.nmode = self.cfg.var.nmode
        self.D = self.cfg.var.ndepth
        self.bn_avg = self.cfg.var.bn_avg
        self.id = id
        self.base_encoder = BaseEncoder(feature_dim=self.feature_dim, multi_scale=True, bn_running_avg=self.bn_avg)
        self.base_decoder = BaseDecoder(int(self.feature_dim), int(self.feature_dim / 2), 3, D=self.D)
        self.conv0 = _conv_lrelu(self.D, self.D)
        self.conv0_1 = _conv_lrelu(self.D, self.D)
        self.conv0_2 = nn.Conv2d(self.D, self.D, kernel_size=3, stride=1, padding=1, bias=True)
        if self.nmode == "default_feedback":
            self.based_3d = Base3D(4, dres_count=2, feature_dim=32, bn_running_avg=self.bn_avg, id=self.id)
        self.apply(_he_init)
        # A reference checkpoint has no entries for Base3D's residual blocks (they sit in a plain Python list there:
        # models.py:394-399).  The reference trainer zips model keys with checkpoint keys and then loads strictly
        # (trainer/base_trainer.py:83-90); these keys are registered LAST here, so the zip drops exactly them, and
        # this hook keeps the strict load from failing on them (they keep their initialisation, as in the reference).
        self.register_load_state_dict_post_hook(_tolerate_missing_dres_blocks)
        self.viz = None
        self.sweep_algo = "auto"  # "direct" selects the gather kernel (debugging / comparison)
        self.packed_epilogue = True   # encoder epilogue kernel + packed sweep entry (False: cat + avg_pool2d + plain entry)
        self.sweep_blas = None    # None = rounding of this host's CPU BLAS; "fma" / "separate" to force
        # how the sweep's backward sums the gradient of the source features: None follows torch.use_deterministic_algorithms(),
        # True / False force the integer sum (reproducible bit for bit) / the float atomics (ops.sweep_cost)
        self.sweep_deterministic = None

    def set_viz(self, viz):
        self.viz = viz

    def freeze_weights(self, name):
        for param in getattr(self, name).parameters():
            param.requires_grad = False

    def weight_init(self, m):
        _he_init(m)

    def init_weights(self):
        self.apply(_he_init)

    # -- feature extraction + batched sweep --------------------------------------------------------
    def _features(self, model_input):
        """(half-resolution features, raw features, sweep features), each [B, V+1, ., ., .].

        The sweep features are the encoder output plus the average-pooled frame (models.py:518-520).  On the default path
        they are never concatenated: the encoder epilogue kernel (ops.pack_views) writes the source views straight into the
        sweep kernels' staging layout and the reference view as NCHW, and `feats` is a _SweepFeatures handle that carries
        both (and still slices like the tensor for the decoder's skip connections, which only read the learned channels)."""
        rgb = model_input["rgb"]
        B, V1 = rgb.shape[0], rgb.shape[1]
        flat = rgb.reshape(B * V1, rgb.shape[2], rgb.shape[3], rgb.shape[4])
        half, raw, feat = self.base_encoder(flat)
        per_view = lambda x: x.view(B, V1, x.shape[1], x.shape[2], x.shape[3])
        feats = None
        if self.sweep_algo == "auto" and self.packed_epilogue and V1 >= 2 and not torch.is_grad_enabled():
            try:
                packed, ref = ops.pack_views(feat.float(), flat.float(), V1, self.D)
                feats = _SweepFeatures(per_view(feat), packed, ref)
            except ops.UnsupportedShape:   # a shape the packed sweep does not take: the concatenated tensor below
                feats = None       # (any other failure of the native call -- launch error, out of memory -- propagates)
        if feats is None:
            rate = int(flat.shape[3] / feat.shape[3])
            # (.float(): under torch.autocast the encoder's maps are fp16 / bf16, the sweep and its backward fp32 only -- a
            # quarter-resolution tensor; fp32 stays itself)
            feats = per_view(torch.cat((feat.float(), F.avg_pool2d(flat, rate)), dim=1))  # [B, V1, C+3, h, w]  (models.py:518-520)
        return per_view(half), per_view(raw), feats

    def _camera(self, model_input):
        K = model_input["intrinsics"].float()
        poses = model_input["src_cam_poses"].float()
        cxcy = K[:, :2, 2].contiguous()  # float32(intrinsic_M[0,2]), float32(intrinsic_M[1,2])  (models.py:538)
        return K, poses, model_input["unit_ray"].float(), cxcy

    def _sweep(self, feats, model_input):
        """cost volume [B, D, h, w]; reference view = last view, sources = the others (models.py:530-534)."""
        K, poses, rays, cxcy = self._camera(model_input)
        R = poses[:, :-1, :3, :3]
        t = poses[:, :-1, :3, 3]
        if isinstance(feats, _SweepFeatures):   # sources already in the staging layout: the packed entry, no pre-pass
            return ops.sweep_cost(feats.ref, feats.packed, K, R, t, rays, cxcy, model_input["d_candi"],
                                  self.sigma_soft_max, feat_dist="L2", algo="auto", blas=self.sweep_blas)
        det = {} if self.sweep_deterministic is None else {"deterministic": self.sweep_deterministic}   # (None: the op's default)
        return ops.sweep_cost(feats[:, -1], feats[:, :-1], K, R, t, rays, cxcy, model_input["d_candi"],
                              self.sigma_soft_max, feat_dist="L2", algo=self.sweep_algo, blas=self.sweep_blas, **det)

    def _low_res_dpv(self, cost_volumes, d_candi, want_prob=False):
        """log-DPV of the cost volume (models.py:555-560); with want_prob also exp(logp) and E[d] from the same pass."""
        x = self.conv0_2(self.conv0_1(self.conv0(cost_volumes)))
        if want_prob:
            # (half logits under torch.autocast: prob in their type, what the decoder's first conv would cast it to anyway)
            lp = {"prob_dtype": x.dtype} if x.dtype in (torch.float16, torch.bfloat16) else {}
            r = ops.dpv_reduce_ex(x, d_candi, want_logp=True, want_prob=True, want_depth=True, inplace=True, **lp)
            return r["logp"], r["prob"], r["depth"]
        logp, _ = ops.dpv_reduce(x, d_candi, want_logp=True, want_depth=False, inplace=True)  # models.py:560
        return logp

    def forward_encoder(self, model_input):
        half, raw, feats = self._features(model_input)
        cost_volumes = self._sweep(feats, model_input)
        BV = self._low_res_dpv(cost_volumes, model_input["d_candi"])
        last = [feats[:, -1, :-3], half[:, -1]]
        first = [feats[:, 0, :-3], half[:, 0]]
        return BV, cost_volumes, last, first

    def forward_exp(self, model_input):
        half, raw, feats = self._features(model_input)
        cost_volumes = self._sweep(feats, model_input)
        K, poses, rays, cxcy = self._camera(model_input)
        # all views incl. the reference (identity pose), channel i warped with plane i (models.py:613-629)
        det = {} if self.sweep_deterministic is None else {"deterministic": self.sweep_deterministic}   # (None: the op's default)
        warped = ops.warp_feature(raw.float(), K, poses[:, :, :3, :3], poses[:, :, :3, 3], rays, cxcy, model_input["d_candi"],
                                  blas=self.sweep_blas, differentiable=True, **det)
        BV = self._low_res_dpv(cost_volumes, model_input["d_candi"])
        last = [feats[:, -1, :-3], half[:, -1]]
        first = [feats[:, 0, :-3], half[:, 0]]
        return BV, cost_volumes, last, first, warped

    def forward_int(self, model_input):
        # self.last_aux: by-products of the DPV passes (depth maps, next prev_output) for harness.eval_step; the
        # returned dict keeps exactly the reference's keys (models.py:656,678,699)
        self.last_aux = None
        d_candi = model_input.get("d_candi")   # (.get: an unknown nmode must reach the reference's error below)
        if self.nmode == "default":
            half, raw, feats_all = self._features(model_input)
            cost_volumes = self._sweep(feats_all, model_input)
            BV_cur, prob, depth_low = self._low_res_dpv(cost_volumes, d_candi, want_prob=True)   # models.py:560 + :651
            feats = [feats_all[:, -1, :-3], half[:, -1], model_input["rgb"][:, -1]]
            BV_refined = self.base_decoder(prob, img_features=feats, d_candi=d_candi)
            self.last_aux = dict(self.base_decoder.aux or {}, depth_lowres=depth_low)
            return {"output": [BV_cur], "output_refined": [BV_refined], "flow": None, "flow_refined": None}
        if self.nmode == "default_upsample":
            BV_cur, _, feats, _ = self.forward_encoder(model_input)
            feats.append(model_input["rgb"][:, -1])
            # gen_dpv_withmask + fuse + renormalise + clamp + log (models.py:663-672) in one kernel
            fused, log_fused = ops.dpv_fuse(BV_cur, model_input["dmaps"], model_input["masks"],
                                            model_input["d_candi"], var=0.3, eps=EPSILON)
            BV_refined = self.base_decoder(fused, img_features=feats)
            return {"output": [log_fused, BV_cur], "output_refined": [BV_refined], "flow": None,
                    "flow_refined": None}
        if self.nmode == "default_feedback":
            BV_cur, _, last, _, warped = self.forward_exp(model_input)
            last.append(model_input["rgb"][:, -1])
            if model_input["prev_output"] is None:
                prev = torch.zeros_like(BV_cur).unsqueeze(1) + 1.0 / float(self.D)
            else:
                prev = model_input["prev_output"].unsqueeze(1)
            resi = self.based_3d(torch.cat([BV_cur.unsqueeze(1), prev, warped], dim=1), prob=False)
            # log_softmax(BV_cur + BV_resi), its exp for the decoder and E[d] in one pass (models.py:694,:697)
            # (.float(): BV_cur is an fp32 log-DPV, and under torch.autocast the 3-D convs' residual is not)
            r = ops.dpv_reduce_ex(BV_cur, d_candi, addend=resi.float().contiguous(), want_logp=True, want_prob=True, want_depth=True)
            BV_upd = r["logp"]
            BV_refined = self.base_decoder(r["prob"], img_features=last, d_candi=d_candi)
            self.last_aux = dict(self.base_decoder.aux or {}, depth_lowres=r["depth"])
            return {"output": [BV_cur, BV_upd], "output_refined": [BV_refined], "flow": None, "flow_refined": None}
        raise Exception("Nmode wrong")

    def forward(self, inputs):
        return [self.forward_int(inp) for inp in inputs]


class DefaultModel(nn.Module):
    """Toy model of the reference (models.py:712-752): two convs + pools, DPV by log_softmax."""

    def __init__(self, cfg, id):
        super().__init__()
        self.cfg = cfg
        self.id = id
        block = lambda cin, cout: nn.Sequential(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=True),
                                                nn.LeakyReLU(0.1, inplace=True))
        self.conv_1x1 = nn.Sequential(block(3, 32), nn.MaxPool2d(2), block(32, self.cfg.var.ndepth), nn.MaxPool2d(2))

    def num_parameters(self):
        return sum(p.data.nelement() if p.requires_grad else 0 for p in self.parameters())

    def init_weights(self):
        for layer in self.modules():
            if isinstance(layer, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(layer.weight)
                if layer.bias is not None:
                    nn.init.constant_(layer.bias, 0)

    def set_viz(self, viz):
        self.viz = viz

    def forward_int(self, input):
        low = self.conv_1x1(input["rgb"][:, -1])
        full = F.interpolate(low, None, 4.0)
        lsm = lambda x: ops.dpv_reduce(x.contiguous(), None, want_logp=True, want_depth=False)[0]
        return {"output": [lsm(low)], "output_refined": [lsm(full)], "flow": None, "flow_refined": None}

    def forward(self, inputs):
        return [self.forward_int(inp) for inp in inputs]
