"""Per-frame visibility feature maps — stays on PyTorch-ROCm ("backbone" side of north_star).

Own PyTorch restatement of the reference's per-frame CNN so that reference checkpoints load by name:
`DepthFusionNet` (conditional_nerf/depth_fusion.py:239-282) = cross-view depth/colour consistency features
(:163-207; on the HIP library, `nl_cross_view_features`) -> `ResEncoder` (conditional_nerf/neuray_ops.py:164-239) + a 2-layer depth skip -> 32-channel map at 1/4
resolution.  It runs once per query frame (not per ray); its output is what `nl_frame_create` receives as
`vis_featmaps`.  With `hip_encode` set, `encode` runs the whole CNN as one call of the fifth HIP library (`nlc_dfnet_forward`, include/nerfloc_cnn.h) wherever no
gradient is wanted; with `hip_training` set, a call whose parameters want gradients runs forward and backward as one autograd node on the eighth library
(`nlct_dfnet_forward_train` / `nlct_dfnet_backward`, include/nerfloc_cnn_train.h).  The default of both is the eager path.  Module/parameter names mirror the reference's state_dict (72 tensors under
`multiview_aggregator.depth_fusion.*`).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from torch.autograd.function import once_differentiable

from . import _packing


def _conv3x3(i, o, stride=1):
    return nn.Conv2d(i, o, 3, stride, 1, bias=False, padding_mode="reflect")


class _BasicBlock(nn.Module):
    """neuray_ops.py:93-131 (InstanceNorm variant)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv3x3(inplanes, planes, stride)
        self.bn1 = nn.InstanceNorm2d(planes, track_running_stats=False, affine=True)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = _conv3x3(planes, planes)
        self.bn2 = nn.InstanceNorm2d(planes, track_running_stats=False, affine=True)
        self.downsample = downsample

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + idn)


class _ConvIN(nn.Module):
    """neuray_ops.py:133-147 — reflect-padded conv + InstanceNorm + ELU."""

    def __init__(self, i, o, k, stride):
        super().__init__()
        self.conv = nn.Conv2d(i, o, k, stride, (k - 1) // 2, padding_mode="reflect")
        self.bn = nn.InstanceNorm2d(o, track_running_stats=False, affine=True)

    def forward(self, x):
        return F.elu(self.bn(self.conv(x)), inplace=True)


class _UpConv(nn.Module):
    """neuray_ops.py:149-157."""

    def __init__(self, i, o, k, scale):
        super().__init__()
        self.scale = scale
        self.conv = _ConvIN(i, o, k, 1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=self.scale, align_corners=True, mode="bilinear"))


class ResEncoder(nn.Module):
    """neuray_ops.py:159-239 — 12-channel input -> 32 channels at 1/4 resolution."""

    def __init__(self):
        super().__init__()
        self.inplanes = 32
        self.conv1 = nn.Conv2d(12, 32, 8, 2, 2, bias=False, padding_mode="reflect")
        self.bn1 = nn.InstanceNorm2d(32, track_running_stats=False, affine=True)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self._layer(32, 2, 2)
        self.layer2 = self._layer(64, 2, 2)
        self.layer3 = self._layer(128, 2, 2)
        self.upconv3 = _UpConv(128, 64, 3, 2)
        self.iconv3 = _ConvIN(128, 64, 3, 1)
        self.upconv2 = _UpConv(64, 32, 3, 2)
        self.iconv2 = _ConvIN(64, 32, 3, 1)
        self.out_conv = nn.Conv2d(32, 32, 1, 1)

    def _layer(self, planes, blocks, stride):
        down = None
        if stride != 1 or self.inplanes != planes:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, stride, bias=False, padding_mode="reflect"),
                                 nn.InstanceNorm2d(planes, track_running_stats=False, affine=True))
        layers = [_BasicBlock(self.inplanes, planes, stride, down)]
        self.inplanes = planes
        layers += [_BasicBlock(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    @staticmethod
    def _skip(x1, x2):
        dy, dx = x2.size(2) - x1.size(2), x2.size(3) - x1.size(3)
        x1 = F.pad(x1, (dx // 2, dx - dx // 2, dy // 2, dy - dy // 2))
        return torch.cat([x2, x1], 1)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x1 = self.layer1(x)
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x = self.iconv3(self._skip(x2, self.upconv3(x3)))
        x = self.iconv2(self._skip(x1, self.upconv2(x)))
        return self.out_conv(x)


class _EncodeTrain(torch.autograd.Function):
    """encode as one node: nlct_dfnet_forward_train keeps the state, nlct_dfnet_backward writes the gradients of the parameters that want one (the others pass NULL).
    cnn_in gets no gradient (the call is taken only where it wants none).  The backward uses the image its forward ran on."""

    @staticmethod
    def forward(ctx, module, cnn_in, *params):
        from . import _cnn_train_lib
        x = cnn_in.detach().contiguous()
        ctx.packed = module._packed_training(x.device, params)
        out, ctx.state = _cnn_train_lib.dfnet_forward_train(ctx.packed, x)
        ctx.x, ctx.shapes, ctx.dtypes = x, [tuple(p.shape) for p in params], [p.dtype for p in params]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        from . import _cnn_train_lib
        grads = _cnn_train_lib.dfnet_backward(ctx.packed, ctx.x, ctx.state, g_out.to(torch.float32).contiguous(), ctx.shapes, ctx.needs_input_grad[2:])
        return (None, None) + tuple(None if g is None else g.to(d) for g, d in zip(grads, ctx.dtypes))


class DepthFusionNet(nn.Module, _packing.PackedCache):
    """depth_fusion.py:239-282 — (imgs, depths, Ks, c2w poses, depth_range) -> (V,32,H/4,W/4)."""

    hip_encode = False   # opt-in, settable per instance: encode() through libnerfloc_cnn.so where it applies (see encode)
    hip_training = False   # opt-in, settable per instance: encode() + its backward through libnerfloc_cnn_train.so where the parameters want gradients

    def __init__(self, cfg=None, in_channels=None):
        super().__init__()
        self.fuse_net = ResEncoder()
        self.depth_skip = nn.Sequential(nn.Conv2d(1, 8, 2, 2), nn.ReLU(True), nn.Conv2d(8, 16, 2, 2))
        self.conv_out = nn.Conv2d(16 + 32, 32, 1, 1)
        self.out_channels = 32
        self._cache_init()
        self._train_cache = _packing.new_train_cache()   # the training image (nlct_dfnet_pack_weights); pack_count counts both images

    def forward(self, imgs, feats, depths, Ks, poses, depth_range):
        """The hand-made input channels (normalised inverse depth + cross-view consistency statistics, reference :150-227) come
        from the HIP library in one pass; the CNN is PyTorch-ROCm (MIOpen), or with `hip_encode` the library's encoder: then nothing eager lies between the two calls."""
        from .frame_setup import cross_view_features
        near, far = [float(x) for x in depth_range.reshape(-1)[:2]]
        return self.encode(cross_view_features(imgs, depths, Ks, poses, near, far))

    def _use_hip(self, cnn_in):
        """The library call is taken only for an fp32 (V, 12, H, W) tensor on a HIP device, inside the library's limits, where no gradient is wanted.  The module's
        train / eval mode does not enter: InstanceNorm without running statistics is the same function in both."""
        if not self.hip_encode or not cnn_in.is_cuda or cnn_in.dtype != torch.float32 or cnn_in.dim() != 4 or cnn_in.shape[1] != 12:
            return False
        if torch.is_grad_enabled() and (cnn_in.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        from . import _cnn_lib
        return _cnn_lib.supported(int(cnn_in.shape[0]), int(cnn_in.shape[2]), int(cnn_in.shape[3]))

    def _encode_hip(self, cnn_in):
        from . import _cnn_lib
        sd = dict(self.named_parameters())
        packed = self._cached(cnn_in.device, [sd[n] for n in _cnn_lib.weight_names()], _cnn_lib.pack_weights)
        return _cnn_lib.dfnet_forward(packed, cnn_in.contiguous())

    def _use_hip_training(self, cnn_in):
        """The training pair is taken only for an fp32 (V, 12, H, W) tensor on a HIP device, inside the library's limits, with grad enabled, where cnn_in itself
        wants no gradient and at least one parameter does."""
        if not self.hip_training or not torch.is_grad_enabled() or not cnn_in.is_cuda or cnn_in.dtype != torch.float32 or cnn_in.dim() != 4 or cnn_in.shape[1] != 12:
            return False
        if cnn_in.requires_grad or not any(p.requires_grad for p in self.parameters()):
            return False
        from . import _cnn_lib
        return _cnn_lib.supported(int(cnn_in.shape[0]), int(cnn_in.shape[2]), int(cnn_in.shape[3]))

    def _packed_training(self, device, params):
        from . import _cnn_train_lib

        def pack(ts):
            self.pack_count += 1
            return _cnn_train_lib.pack_weights(ts)
        return self._train_cache._cached(device, list(params), pack)

    def _encode_hip_training(self, cnn_in):
        from . import _cnn_lib
        sd = dict(self.named_parameters())
        return _EncodeTrain.apply(self, cnn_in, *[sd[n] for n in _cnn_lib.weight_names()])

    def encode(self, cnn_in):
        """(V,12,H,W) = [rgb | normalised inverse depth | 8 consistency channels] -> (V,32,H/4,W/4) (reference :279-282).  The path is chosen per call."""
        if self._use_hip(cnn_in):
            return self._encode_hip(cnn_in)
        if self._use_hip_training(cnn_in):
            return self._encode_hip_training(cnn_in)
        x = self.fuse_net(cnn_in)
        return self.conv_out(torch.cat([self.depth_skip(cnn_in[:, 3:4]), x], 1))
