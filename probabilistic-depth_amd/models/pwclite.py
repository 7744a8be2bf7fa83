"""PWCLite, the flow network of the reference's models/pwclite.py, with its constructor contract (cfg.upsample, cfg.n_frames,
cfg.reduce_dense), its forward(x, with_bk=False) -> {'flows_fw', 'flows_bw'}, num_parameters, init_weights, and its module and
parameter names -- state_dict() keys and shapes are the reference's, so its checkpoints load:
    feature_pyramid_extractor.convs.<l>.<0|1>.0    six levels, each a stride-2 and a stride-1 3x3 convolution (16 ... 192 channels)
    flow_estimators.conv1 .. conv5 + conv_last     (dense) / + predict_flow (reduce), shared by every level
    context_networks.convs.<0..6>.0                the dilated refinement
    conv_1x1.<l>.0                                 a level's features squeezed to 32 channels
The convolutions are PyTorch's.  The one other hot path is the per-level cost volume
    leaky_relu(correlation(x1, flow_warp(x2, flow)), 0.1)          (no warp at the coarsest level)
which with fused_cost=True and fp32 device tensors is ONE HIP pass, ops.flow_cost_volume (csrc/cost_volume.hip: the warped features
and the pre-activation volume are never written), and otherwise the composition of warp_utils.flow_warp, the correlation and
F.leaky_relu: the HIP ops on fp32 device tensors, plain torch anywhere else (CPU tensors, other dtypes).  fused_cost is off by
default: measured on the whole model, forward and backward, the fused pass was 1.3 % slower than the composition.
Five levels are estimated, coarse to fine, each starting from the level before upsampled by two; the flows are returned finest
first, at a quarter of the input's resolution or, with cfg.upsample, at the input's.  Nothing is printed.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..utils.warp_utils import _on_hip, flow_warp

SLOPE = 0.1


def conv(in_planes, out_planes, kernel_size=3, stride=1, dilation=1, isReLU=True):
    """Conv2d ('same' padding for the dilation) [+ LeakyReLU(0.1)] as a Sequential: the convolution is module 0."""
    layers = [nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, dilation=dilation,
                        padding=((kernel_size - 1) * dilation) // 2, bias=True)]
    if isReLU:
        layers.append(nn.LeakyReLU(SLOPE, inplace=True))
    return nn.Sequential(*layers)


class FeatureExtractor(nn.Module):
    def __init__(self, num_chs):
        super().__init__()
        self.num_chs = num_chs
        self.convs = nn.ModuleList(nn.Sequential(conv(a, b, stride=2), conv(b, b)) for a, b in zip(num_chs[:-1], num_chs[1:]))

    def forward(self, x):
        """-> the levels' features, coarsest first."""
        pyramid = []
        for level in self.convs:
            x = level(x)
            pyramid.append(x)
        return pyramid[::-1]


class FlowEstimatorDense(nn.Module):
    """Five convolutions, each reading everything before it; feat_dim = ch_in + 448."""

    def __init__(self, ch_in):
        super().__init__()
        widths = (128, 128, 96, 64, 32)
        for i, w in enumerate(widths):
            setattr(self, "conv%d" % (i + 1), conv(ch_in + sum(widths[:i]), w))
        self.feat_dim = ch_in + sum(widths)
        self.conv_last = conv(self.feat_dim, 2, isReLU=False)

    def forward(self, x):
        for layer in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
            x = torch.cat([layer(x), x], dim=1)
        return x, self.conv_last(x)


class FlowEstimatorReduce(nn.Module):
    """The lighter estimator: each convolution reads the two results before it; feat_dim = 32."""

    def __init__(self, ch_in):
        super().__init__()
        self.conv1 = conv(ch_in, 128)
        self.conv2 = conv(128, 128)
        self.conv3 = conv(128 + 128, 96)
        self.conv4 = conv(128 + 96, 64)
        self.conv5 = conv(96 + 64, 32)
        self.feat_dim = 32
        self.predict_flow = conv(64 + 32, 2, isReLU=False)

    def forward(self, x):
        x1 = self.conv1(x)
        x2 = self.conv2(x1)
        x3 = self.conv3(torch.cat([x1, x2], dim=1))
        x4 = self.conv4(torch.cat([x2, x3], dim=1))
        x5 = self.conv5(torch.cat([x3, x4], dim=1))
        return x5, self.predict_flow(torch.cat([x4, x5], dim=1))


class ContextNetwork(nn.Module):
    def __init__(self, ch_in):
        super().__init__()
        plan = ((ch_in, 128, 1), (128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1))
        self.convs = nn.Sequential(*[conv(a, b, 3, 1, d) for a, b, d in plan], conv(32, 2, isReLU=False))

    def forward(self, x):
        return self.convs(x)


def correlation(x1, x2, max_displacement):
    """The correlation of the network's configuration (kernel 1, strides 1, pad_size = max_displacement): ops.correlation on fp32
    device tensors, else the padded shift-multiply-mean in plain torch, channel (tj + md)(2 md + 1) + (ti + md), tj the row."""
    md = max_displacement
    if _on_hip(x1, x2):
        return ops.correlation(x1, x2, md, 1, md, 1, 1, 1)
    H, W = x1.shape[2:]
    padded = F.pad(x2, [md] * 4)
    return torch.cat([(x1 * padded[:, :, i:i + H, j:j + W]).mean(1, keepdim=True)
                      for i in range(2 * md + 1) for j in range(2 * md + 1)], 1)


def _up(flow, factor):
    return F.interpolate(flow * factor, scale_factor=factor, mode='bilinear', align_corners=True)


class PWCLite(nn.Module):
    def __init__(self, cfg, fused_cost=False):
        super().__init__()
        self.search_range = 4
        self.num_chs = [3, 16, 32, 64, 96, 128, 192]
        self.output_level = 4
        self.num_levels = 7
        self.fused_cost = bool(fused_cost)
        self.upsample = cfg.upsample
        self.n_frames = cfg.n_frames
        self.reduce_dense = cfg.reduce_dense

        self.feature_pyramid_extractor = FeatureExtractor(self.num_chs)
        self.dim_corr = (self.search_range * 2 + 1) ** 2
        self.num_ch_in = 32 + (self.dim_corr + 2) * (self.n_frames - 1)
        estimator = FlowEstimatorReduce if self.reduce_dense else FlowEstimatorDense
        self.flow_estimators = estimator(self.num_ch_in)
        self.context_networks = ContextNetwork((self.flow_estimators.feat_dim + 2) * (self.n_frames - 1))
        self.conv_1x1 = nn.ModuleList(conv(c, 32, kernel_size=1) for c in self.num_chs[:1:-1])

    def num_parameters(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def cost_volume(self, x1, x2, flow=None):
        """leaky_relu(correlation(x1, flow_warp(x2, flow)), 0.1), [B,81,h,w]; flow None: no warp."""
        if self.fused_cost and _on_hip(x1, x2) and (flow is None or _on_hip(flow)):
            return ops.flow_cost_volume(x1, x2, flow, max_displacement=self.search_range, negative_slope=SLOPE, pad='border')
        warped = x2 if flow is None else flow_warp(x2, flow)
        return F.leaky_relu(correlation(x1, warped, self.search_range), SLOPE)

    def _finish(self, flows):
        if self.upsample:
            flows = [_up(f, 4) for f in flows]
        return flows[::-1]

    def forward_2_frames(self, x1_pyramid, x2_pyramid):
        """-> the flows 1 -> 2 of the five levels, finest first."""
        flows, flow = [], None
        for l, (x1, x2) in enumerate(zip(x1_pyramid, x2_pyramid)):
            if l == 0:
                flow = torch.zeros((x1.shape[0], 2) + tuple(x1.shape[2:]), dtype=torch.float32, device=x1.device)
                cost = self.cost_volume(x1, x2)
            else:
                flow = _up(flow, 2)
                cost = self.cost_volume(x1, x2, flow)
            feat, residual = self.flow_estimators(torch.cat([cost, self.conv_1x1[l](x1), flow], dim=1))
            flow = flow + residual
            flow = flow + self.context_networks(torch.cat([feat, flow], dim=1))
            flows.append(flow)
            if l == self.output_level:
                break
        return self._finish(flows)

    def forward_3_frames(self, x0_pyramid, x1_pyramid, x2_pyramid):
        """-> (flows 1 -> 0, flows 1 -> 2), each finest first.  A level's flow carries both: channels 0:2 towards frame 0, 2:4
        towards frame 2; the estimator and the refinement run once per direction, each seeing its own direction first and the
        other's flow negated."""
        flows, flow = [], None
        for l, (x0, x1, x2) in enumerate(zip(x0_pyramid, x1_pyramid, x2_pyramid)):
            if l == 0:
                flow = torch.zeros((x1.shape[0], 4) + tuple(x1.shape[2:]), dtype=torch.float32, device=x1.device)
                cost_10, cost_12 = self.cost_volume(x1, x0), self.cost_volume(x1, x2)
            else:
                flow = _up(flow, 2)
                cost_10, cost_12 = self.cost_volume(x1, x0, flow[:, :2]), self.cost_volume(x1, x2, flow[:, 2:])
            squeezed = self.conv_1x1[l](x1)
            f10, f12 = flow[:, :2], flow[:, 2:]
            feat_10, res_10 = self.flow_estimators(torch.cat([squeezed, cost_10, cost_12, f10, -f12], dim=1))
            feat_12, res_12 = self.flow_estimators(torch.cat([squeezed, cost_12, cost_10, f12, -f10], dim=1))
            flow = flow + torch.cat([res_10, res_12], dim=1)
            f10, f12 = flow[:, :2], flow[:, 2:]
            res_10 = self.context_networks(torch.cat([feat_10, feat_12, f10, -f12], dim=1))
            res_12 = self.context_networks(torch.cat([feat_12, feat_10, f12, -f10], dim=1))
            flow = flow + torch.cat([res_10, res_12], dim=1)
            flows.append(flow)
            if l == self.output_level:
                break
        flows = self._finish(flows)
        return [f[:, :2] for f in flows], [f[:, 2:] for f in flows]

    def forward(self, x, with_bk=False):
        """x [B, 3 n, H, W], n = 2, 3 or 5 frames -> {'flows_fw': ..., 'flows_bw': ...} (2 frames: flows_bw only with_bk; 5 frames:
        a list per centre frame)."""
        n_frames = x.size(1) // 3
        if x.size(1) != 3 * n_frames or n_frames not in (2, 3, 5):
            raise NotImplementedError("PWCLite takes 2, 3 or 5 frames of 3 channels, got %d channels" % x.size(1))
        pyramids = []
        for i in range(n_frames):
            img = x[:, 3 * i:3 * i + 3]
            pyramids.append(self.feature_pyramid_extractor(img) + [img])
        res = {}
        if n_frames == 2:
            res['flows_fw'] = self.forward_2_frames(pyramids[0], pyramids[1])
            if with_bk:
                res['flows_bw'] = self.forward_2_frames(pyramids[1], pyramids[0])
        elif n_frames == 3:
            flows_10, flows_12 = self.forward_3_frames(*pyramids)
            res['flows_fw'], res['flows_bw'] = flows_12, flows_10
        else:
            flows_10, flows_12 = self.forward_3_frames(*pyramids[0:3])
            flows_21, flows_23 = self.forward_3_frames(*pyramids[1:4])
            res['flows_fw'] = [flows_12, flows_23]
            if with_bk:
                flows_32, flows_34 = self.forward_3_frames(*pyramids[2:5])
                res['flows_bw'] = [flows_21, flows_32]
        return res
