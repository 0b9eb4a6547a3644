"""Drop-ins for the reference's models/appearance_embedding.py: AppearanceEmbedding and AppearanceAdaptLayer on libnerfloc_app.so (include/nerfloc_app.h).

Same constructors, same state-dict names and shapes, same call signatures and return shapes: a NeRF-Loc checkpoint's `adapt_appearance_*.*` loads with strict=True
and `from nerf_loc_amd.appearance import AppearanceEmbedding, AppearanceAdaptLayer` replaces the reference's import.  On fp32 HIP tensors the statistics, the
adaptation MLP (eval) and the per-channel affine rewrite with its gradients run in the library; CPU tensors, other dtypes and `hip_training = False` run the
reference's formulation in eager PyTorch.  There is no silent fallback for a missing library: the library path raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _app_lib


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class AppearanceEmbedding(nn.Module):
    """forward(imgs, x): x['conv1'] (B, c, H, W) -> (B, 2 c): each channel's mean, then its unbiased standard deviation.  No parameters.

    fp32 HIP tensor, no gradient wanted: ONE nla_channel_stats call for all B images; NCHW-contiguous and channels_last maps are read as they lie, anything else
    costs one copy.  CPU tensors, other dtypes, or a `conv1` that requires grad (with grad enabled) take the eager formulation (torch.std_mean).  The library has
    no backward for the statistics on purpose: the reference freezes the backbone's conv1 (its backbone2d.py sets requires_grad_(False) on it), so no training run
    differentiates this embedding.
    hip_eval (attribute): False selects the eager formulation on HIP tensors too (tools/appearance_bench.py times the two against each other).
    """
    hip_eval = True

    def __init__(self, args):
        super().__init__()
        self.dim = args.appearance_emb_dim

    def forward(self, imgs, x):
        conv1 = x["conv1"]
        assert 2 * conv1.shape[1] == self.dim
        if not self.hip_eval or not conv1.is_cuda or conv1.dtype != torch.float32 or _wants_grad(conv1):
            std, mean = torch.std_mean(conv1.reshape(conv1.shape[0], conv1.shape[1], -1), dim=2)
            return torch.cat([mean, std], dim=1)
        conv1 = conv1.detach()
        if not conv1.is_contiguous() and not conv1.is_contiguous(memory_format=torch.channels_last):
            conv1 = conv1.contiguous()
        return _app_lib.channel_stats(conv1)


class _FilmFn(torch.autograd.Function):
    """y = code[:, :C] * x + code[:, C:] (clamped to [0, 1] with clip) as ONE node: saves x and the (V, 2 C) code, nothing else of the map's size."""

    @staticmethod
    def forward(ctx, x, code, clip):
        x, code = x.contiguous(), code.contiguous()
        ctx.clip = bool(clip)
        ctx.save_for_backward(x, code)
        return _app_lib.film(x, code, ctx.clip)

    @staticmethod
    @torch.autograd.function.once_differentiable   # a second-order backward raises
    def backward(ctx, g_y):
        x, code = ctx.saved_tensors
        want_x, want_code = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_code):
            return None, None, None
        g_x, g_code = _app_lib.film_backward(x, code, g_y.contiguous(), ctx.clip, want_x, want_code)
        return g_x, g_code, None


class AppearanceAdaptLayer(nn.Module):
    """forward(x (B, H, W, C), embedding (B, E), target_embedding (1, E) or (E,)) -> (B, H, W, C): a * x + b per channel with (a | b) = mlp(target - embedding);
    clamped to [0, 1] with is_rgb.  State dict: mlp.{0,2,4}.{weight,bias}, as the reference.

    fp32 HIP tensors, no gradient wanted (nothing requires grad, or grad is disabled): nla_adapt_code + nla_film, two launches.  A gradient is wanted (training mode
    or an input / parameter that requires grad): the code comes from the eager `self.mlp` (B rows: autograd owns the MLP) and the rewrite is one autograd node around
    nla_film / nla_film_backward, which passes NULL for a cotangent nobody wants; a second-order backward raises.  Non-contiguous x costs one copy.
    hip_training (attribute): False selects the eager formulation wherever a gradient is wanted (as S2DMatching.hip_training); hip_eval: the same switch for the path
    without a gradient.  CPU tensors and other dtypes always take the eager formulation.
    """
    hip_training = True
    hip_eval = True

    def __init__(self, args, input_dim, is_rgb=False):
        super().__init__()
        self.input_dim = input_dim
        self.appearance_emb_dim = args.appearance_emb_dim
        self.is_rgb = is_rgb
        self.mlp = nn.Sequential(
            nn.Linear(self.appearance_emb_dim, 64),
            nn.LeakyReLU(inplace=True),
            nn.Linear(64, 64),
            nn.LeakyReLU(inplace=True),
            nn.Linear(64, input_dim * 2),
        )

    def _eager(self, x, embedding, target_embedding):
        code = self.mlp(target_embedding - embedding)
        a, b = torch.split(code, [self.input_dim, self.input_dim], dim=-1)
        y = a[:, None, None, :] * x + b[:, None, None, :]
        return torch.clip(y, min=0.0, max=1.0) if self.is_rgb else y

    def forward(self, x, embedding, target_embedding):
        params = list(self.mlp.parameters())
        tensors = [x, embedding, target_embedding] + params
        on_hip = all(t.is_cuda and t.dtype == torch.float32 for t in tensors)
        wanted = torch.is_grad_enabled() and (self.training or any(t.requires_grad for t in tensors))
        if not on_hip or not (self.hip_training if wanted else self.hip_eval):
            return self._eager(x, embedding, target_embedding)
        if wanted:
            code = self.mlp(target_embedding - embedding)
            if code.dim() == 1:
                code = code[None]
            return _FilmFn.apply(x, code, self.is_rgb)
        emb = embedding.detach().contiguous()
        if emb.dim() == 1:
            emb = emb[None]
        code = _app_lib.adapt_code(emb, target_embedding.detach().reshape(-1).contiguous(), [p.detach().contiguous() for p in params])
        return _app_lib.film(x.detach().contiguous(), code, self.is_rgb)
