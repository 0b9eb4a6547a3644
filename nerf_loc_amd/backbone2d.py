"""The 2-D backbone: ResNet-50 with frozen BatchNorm up to the last requested layer, plus an optional feature pyramid with InstanceNorm.

Own PyTorch restatement of the reference's `models/COTR/backbone2d.py` (+ `resnet.py`, `fpn.py`) so that reference checkpoints load by name and nothing outside
torch is needed: the reference takes `transforms.Normalize` and `IntermediateLayerGetter` from torchvision, here the normalisation is two buffers-free constants
and the layer getter is `_Body`, a ModuleDict that holds the ResNet's children up to the last returned one and walks them in order.  The eager path is plain
`torch.nn`, runs on CPU and GPU and is what training uses.  With `hip_forward` set, the configuration the pose estimator ships
(`return_layers=['conv1', 'layer1', 'layer2']`, `use_fpn=True`) runs as one call of the sixth HIP library (`nlb_backbone_forward`, include/nerfloc_backbone.h)
wherever no gradient is wanted; the default is the eager path.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _packing

IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)
HIP_RETURN_LAYERS = ["conv1", "layer1", "layer2"]
HIP_FPN_DIMS = (64, 128, 192, 256)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d whose statistics and affine parameters are buffers: y = x * scale + bias with scale = weight * rsqrt(running_var + 1e-5) and
    bias = bias - running_mean * scale.  A checkpoint's `num_batches_tracked` is dropped on load."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x):
        scale = self.weight.reshape(1, -1, 1, 1) * (self.running_var.reshape(1, -1, 1, 1) + 1e-5).rsqrt()
        bias = self.bias.reshape(1, -1, 1, 1) - self.running_mean.reshape(1, -1, 1, 1) * scale
        return x * scale + bias


class _Bottleneck(nn.Module):
    """1 x 1 -> 3 x 3 (carries the stride) -> 1 x 1 to 4 x planes, each followed by a frozen BN; ReLU(bn3(conv3) + identity)."""

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = FrozenBatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(4 * planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + idn)


def _resnet50_children():
    """The ResNet-50's children in order: conv1, bn1, relu, maxpool, layer1 .. layer4 (3, 4, 6, 3 bottlenecks of 64, 128, 256, 512 planes)."""
    mods = OrderedDict()
    mods["conv1"] = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    mods["bn1"] = FrozenBatchNorm2d(64)
    mods["relu"] = nn.ReLU(inplace=True)
    mods["maxpool"] = nn.MaxPool2d(3, 2, 1)
    inplanes = 64
    for i, (planes, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), start=1):
        stride = 1 if i == 1 else 2
        down = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride, bias=False), FrozenBatchNorm2d(4 * planes))
        layers = [_Bottleneck(inplanes, planes, stride, down)]
        inplanes = 4 * planes
        layers += [_Bottleneck(inplanes, planes) for _ in range(1, blocks)]
        mods[f"layer{i}"] = nn.Sequential(*layers)
    for m in mods.values():
        for c in m.modules():
            if isinstance(c, nn.Conv2d):
                nn.init.kaiming_normal_(c.weight, mode="fan_out", nonlinearity="relu")
    return mods


class _Body(nn.ModuleDict):
    """The children of the ResNet up to the last one in `return_layers`; forward walks them in order and returns the named ones' outputs."""

    def __init__(self, children, return_layers):
        missing = [l for l in return_layers if l not in children]
        if missing:
            raise ValueError(f"return_layers {missing} are not present in the model")
        left, kept = set(return_layers), OrderedDict()
        for name, m in children.items():
            kept[name] = m
            left.discard(name)
            if not left:
                break
        super().__init__(kept)
        self.return_layers = set(return_layers)

    def forward(self, x):
        out = OrderedDict()
        for name, m in self.items():
            x = m(x)
            if name in self.return_layers:
                out[name] = x
        return out


class _FPN(nn.Module):
    """Top-down pyramid: per level a 1 x 1 `inner` and a 3 x 3 `layer` convolution, bias-free, each followed by a non-affine InstanceNorm; the coarser level's inner
    map is resized with nearest neighbour to the finer one's size and added to it."""

    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        self.inner_blocks = nn.ModuleList()
        self.layer_blocks = nn.ModuleList()
        for c in in_channels_list:
            if c == 0:
                raise ValueError("in_channels=0 is currently not supported")
            self.inner_blocks.append(nn.Sequential(nn.Conv2d(c, out_channels, 1, bias=False), nn.InstanceNorm2d(out_channels)))
            self.layer_blocks.append(nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.InstanceNorm2d(out_channels)))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)

    def forward(self, x):
        names, maps = list(x.keys()), list(x.values())
        last = self.inner_blocks[-1](maps[-1])
        results = [self.layer_blocks[-1](last)]
        for i in range(len(maps) - 2, -1, -1):
            lateral = self.inner_blocks[i](maps[i])
            last = lateral + F.interpolate(last, size=lateral.shape[-2:], mode="nearest")
            results.insert(0, self.layer_blocks[i](last))
        return OrderedDict(zip(names, results))


class Backbone(nn.Module, _packing.PackedCache):
    """images (B, 3, H, W) in [0, 1] -> OrderedDict of the requested layers' maps; with `use_fpn` the `layer*` entries are the pyramid's outputs, `conv1` stays the
    raw convolution output (before bn1)."""

    hip_forward = False                   # opt-in, settable per instance: forward() through libnerfloc_backbone.so where it applies (see _use_hip)
    hip_precision = "fp32"                # the precision of the library call
    hip_output_layout = "channels_last"   # the FPN maps of the library call: (B, C, h, w) in NHWC memory, or "nchw": dense NCHW

    def __init__(self, return_layers, train_backbone=True, use_fpn=False, fpn_dim=128):
        super().__init__()
        self.layer_to_channels = {"conv1": 64, "layer1": 256, "layer2": 512, "layer3": 1024, "layer4": 2048}
        self.layer_to_stride = {"conv1": 2, "layer1": 4, "layer2": 8, "layer3": 16, "layer4": 32}
        self.return_layers = return_layers
        children = _resnet50_children()
        for name, m in children.items():
            if not train_backbone or name not in ("layer2", "layer3", "layer4"):
                for p in m.parameters():
                    p.requires_grad_(False)
        self.body = _Body(children, return_layers)
        self.use_fpn = use_fpn
        self.fpn_dim = fpn_dim
        if use_fpn:
            self.fpn = _FPN([self.layer_to_channels[l] for l in return_layers if "layer" in l], fpn_dim)
            self.layer_to_channels.update({l: fpn_dim for l in return_layers if "layer" in l})
        self._cache_init()

    def normalize(self, x):
        mean = torch.tensor(IMAGE_MEAN, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        std = torch.tensor(IMAGE_STD, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        return (x - mean) / std

    def _use_hip(self, x):
        """The library call is taken only in the shipped configuration, for an fp32 (B, 3, H, W) tensor on a HIP device inside the library's limits, where no
        gradient is wanted.  Train / eval mode does not enter: frozen BN and InstanceNorm without running statistics are the same function in both."""
        if not self.hip_forward or not self.use_fpn or list(self.return_layers) != HIP_RETURN_LAYERS or self.fpn_dim not in HIP_FPN_DIMS:
            return False
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        from . import _backbone_lib
        return _backbone_lib.supported(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), self.fpn_dim)

    def _forward_hip(self, x):
        from . import _backbone_lib
        sd = self.state_dict(keep_vars=True)
        packed = self._cached(x.device, [sd[n] for n in _backbone_lib.weight_names()], lambda ts: _backbone_lib.pack_weights(ts, self.fpn_dim))
        c1, p1, p2 = _backbone_lib.backbone_forward(packed, x.contiguous(), self.fpn_dim, precision=self.hip_precision, layout=self.hip_output_layout)
        return OrderedDict((("conv1", c1), ("layer1", p1), ("layer2", p2)))

    def forward(self, x):
        """The path is chosen per call."""
        if self._use_hip(x):
            return self._forward_hip(x)
        y = self.body(self.normalize(x))
        if self.use_fpn:
            y.update(self.fpn(OrderedDict((l, y[l]) for l in self.return_layers if "layer" in l)))
        return y


def build_backbone(model_path="models/COTR/default/checkpoint.pth.tar", return_layers=["layer1", "layer2", "layer3", "layer4"], train_backbone=True, use_fpn=False,
                   fpn_dim=128):
    """A Backbone with the `backbone.0.*` tensors of a COTR checkpoint loaded (non-strict: the checkpoint has no pyramid and may hold layers that are not kept)."""
    ckpt = torch.load(model_path)
    state_dict = {k.replace("backbone.0.", ""): v for k, v in ckpt["model_state_dict"].items() if "backbone" in k}
    backbone = Backbone(return_layers=return_layers, train_backbone=train_backbone, use_fpn=use_fpn, fpn_dim=fpn_dim)
    backbone.load_state_dict(state_dict, strict=False)
    return backbone
