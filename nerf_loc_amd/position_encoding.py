"""Drop-ins for the two position encodings of the reference's localisation head: `PositionEmbeddingSine` (models/COTR/position_encoding.py:53-80, used on the coarse
map and on the 7 x 7 fine windows) and `get_embedder` (models/conditional_nerf/utils.py:38-53, the NeRF embedder the head applies to pts3d_ndc).

On HIP tensors both are library calls (csrc/head.hip: nlh_pos_sine_grid, nlh_embed_points).  The sine table of a map depends on its (H, W) and C alone, so it is
computed once per shape and device, cached, and expanded over the batch: a view, no copy and no launch on later frames.  On CPU tensors both are the eager
formulation, which is also what the GPU kernels are tested against.  `exp_sine` and `include_input=True` stay eager everywhere.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _head_lib

_TABLES = {}   # (H, W, C, device) -> the (H, W, C) table; shared by every PositionEmbeddingSine (the values depend on nothing else)


def sine_table(H, W, C, device):
    """The cached (H, W, C) fp32 lin_sine table on a HIP device (nlh_pos_sine_grid on the first use of a shape)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("sine_table: the library's table lives on a HIP device; CPU tensors take the eager formulation")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(H), int(W), int(C), device.index)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = _head_lib.pos_sine_grid(H, W, C, device)
    return t


class NerfPositionalEncoding(nn.Module):
    """sin(b pi x) for every base b, then cos(b pi x): out_dim = in_dim * depth * 2 (eager)."""

    def __init__(self, depth=10, sine_type="lin_sine"):
        super().__init__()
        if sine_type == "lin_sine":
            self.bases = [i + 1 for i in range(depth)]
        elif sine_type == "exp_sine":
            self.bases = [2 ** i for i in range(depth)]
        else:
            raise ValueError(f"not supported {sine_type}")

    @torch.no_grad()
    def forward(self, inputs):
        return torch.cat([torch.sin(i * math.pi * inputs) for i in self.bases] + [torch.cos(i * math.pi * inputs) for i in self.bases], dim=-1)


class PositionEmbeddingSine(nn.Module):
    """`PositionEmbeddingSine(num_pos_feats, temperature, normalize, scale, sine_type)` with the reference's constructor; forward(x: (B, H, W)) -> (B, H, W, C),
    C = 2 * num_pos_feats.  No parameters.  The result depends on x's shape alone; on a HIP tensor with lin_sine it is an expanded view of the cached table."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None, sine_type="lin_sine"):
        super().__init__()
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.normalize = normalize
        self.sine_type = sine_type
        self.sine = NerfPositionalEncoding(num_pos_feats // 2, sine_type)

    @property
    def channels(self):
        return 4 * (self.num_pos_feats // 2)

    @torch.no_grad()
    def _eager(self, x):
        mask = torch.ones_like(x)
        y_embed = mask.cumsum(1, dtype=torch.float32)
        x_embed = mask.cumsum(2, dtype=torch.float32)
        eps = 1e-6
        y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps)
        x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps)
        return self.sine(torch.stack([x_embed, y_embed], dim=-1))

    @torch.no_grad()
    def forward(self, x):
        if x.dim() != 3:
            raise ValueError("PositionEmbeddingSine: x must be (B, H, W)")
        B, H, W = x.shape
        if x.is_cuda and self.sine_type == "lin_sine" and self.channels >= 4 and H >= 1 and W >= 1:
            return sine_table(H, W, self.channels, x.device).unsqueeze(0).expand(B, H, W, self.channels)
        return self._eager(x)


def get_embedder(multires, i=0, include_input=False):
    """(fn, out_dim) as the reference's get_embedder for 3-D inputs: log-sampled frequencies 2^0 .. 2^(multires - 1), per frequency sin then cos.  On HIP tensors
    (and include_input=False) fn is nlh_embed_points, whose full-range sine is needed at 2^31 |x|; otherwise it is eager."""
    if i == -1:
        return nn.Identity(), 3
    L = int(multires)
    freqs = 2.0 ** torch.linspace(0.0, L - 1, steps=L)
    out_dim = 3 * 2 * L + (3 if include_input else 0)

    def eager(x):
        parts = [x] if include_input else []
        for f in freqs:
            parts += [torch.sin(x * f), torch.cos(x * f)]   # f: a 0-d CPU tensor, taken as a number on any device
        return torch.cat(parts, -1)

    def embed(x):
        if x.is_cuda and not include_input and 1 <= L <= 32 and x.shape[-1] <= 64:
            return _head_lib.embed_points(x, L)
        return eager(x)
    embed.eager = eager   # the eager formulation on any device (tools/head_bench.py times it as the baseline)
    return embed, out_dim
