"""A stand-in for the two torchvision names the reference's backbone2d.py imports, for machines without torchvision (tools/gen_backbone_golden.py).

Written from torchvision's documented behaviour, not from its source:
  torchvision.transforms.Normalize(mean, std): a module; forward(tensor (..., C, H, W)) returns a new tensor with
      output[channel] = (input[channel] - mean[channel]) / std[channel], mean and std taken in the tensor's dtype; the input is not modified.
  torchvision.models._utils.IntermediateLayerGetter(model, return_layers): a ModuleDict of the model's direct children, in registration order, up to and
      including the last one named in return_layers (a dict: child name -> output name); a name that is no child raises ValueError; forward(x) applies the
      children in order and returns an OrderedDict of the named children's outputs under their output names.
install() registers modules under those names in sys.modules.
"""
import sys
import types
from collections import OrderedDict

import torch
from torch import nn


class Normalize(nn.Module):
    def __init__(self, mean, std, inplace=False):
        super().__init__()
        self.mean, self.std = list(mean), list(std)

    def forward(self, tensor):
        mean = torch.as_tensor(self.mean, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
        return (tensor - mean) / std


class IntermediateLayerGetter(nn.ModuleDict):
    def __init__(self, model, return_layers):
        if not set(return_layers).issubset(name for name, _ in model.named_children()):
            raise ValueError("return_layers are not present in model")
        left = dict(return_layers)
        layers = OrderedDict()
        for name, module in model.named_children():
            layers[name] = module
            left.pop(name, None)
            if not left:
                break
        super().__init__(layers)
        self.return_layers = dict(return_layers)

    def forward(self, x):
        out = OrderedDict()
        for name, module in self.items():
            x = module(x)
            if name in self.return_layers:
                out[self.return_layers[name]] = x
        return out


def install():
    mods = {name: types.ModuleType(name) for name in ("torchvision", "torchvision.transforms", "torchvision.models", "torchvision.models._utils")}
    mods["torchvision"].transforms, mods["torchvision"].models = mods["torchvision.transforms"], mods["torchvision.models"]
    mods["torchvision.models"]._utils = mods["torchvision.models._utils"]
    mods["torchvision.transforms"].Normalize = Normalize
    mods["torchvision.models._utils"].IntermediateLayerGetter = IntermediateLayerGetter
    sys.modules.update(mods)
