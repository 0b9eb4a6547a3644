"""Drop-in for the reference's `SelfCrossTransformer` (models/COTR/transformer.py:17-64, used twice by matcher.py: coarse :68-72 and fine :120-124).

Eval mode on a HIP device is ONE library call (nl_sct_forward, csrc/sct.hip): four post-norm layers, each a projection kernel, a flash-style attention kernel that
never writes an Nq x Nk tensor, and a row-chain kernel (out_proj, residual, LayerNorm, FFN, residual, LayerNorm) whose hidden rows stay on chip.  Training mode, or
an input that requires grad while grad is enabled, runs the same four layers in eager PyTorch through the same sub-modules (plumbing so that swapping the class does
not break a training script; there is no gradient kernel).  Eval mode on CPU tensors is refused: no CPU fallback.

The sub-modules carry the reference's names (`self_attn_layer{0,1}.self_attn / linear1 / linear2 / norm1 / norm2`, `cross_attn_layer{0,1}.multihead_attn /
linear1 / linear2 / norm1 / norm2 / norm3`), so `matcher.coarse_transformer.*` and `matcher.fine_transformer.*` of a NeRF-Loc checkpoint load with strict=True.
The decoder layers' norm1 is constructed and never applied, as in the reference.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._packing import PackedCache, check_precision, require_device

_LIMITS = "nhead == 8, d_model in {64, 128, 192, 256}, dim_feedforward a multiple of 32 in 32..512, activation 'relu'"


class _Layer(nn.Module):
    """One post-norm layer: attention (q = x + pos_x, k = mem + pos_mem, value = mem), residual, LayerNorm, FFN, residual, LayerNorm."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout, cross):
        super().__init__()
        attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        if cross:
            self.multihead_attn = attn
        else:
            self.self_attn = attn
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        if cross:
            self.norm3 = nn.LayerNorm(d_model)
            self.dropout1 = nn.Dropout(dropout)   # constructed and unused, like norm1 (the reference's decoder layer)
        self.dropout_a = nn.Dropout(dropout)
        self.dropout_b = nn.Dropout(dropout)
        self.cross = cross

    def forward(self, x, pos_x, mem, pos_mem):   # sequence first
        attn = self.multihead_attn if self.cross else self.self_attn
        norm_a, norm_b = (self.norm2, self.norm3) if self.cross else (self.norm1, self.norm2)
        a = attn(x + pos_x, mem + pos_mem, mem, need_weights=False)[0]
        x = norm_a(x + self.dropout_a(a))
        f = self.linear2(self.dropout(F.relu(self.linear1(x))))
        return norm_b(x + self.dropout_b(f))


class SelfCrossTransformer(nn.Module, PackedCache):
    """`SelfCrossTransformer(d_model, nhead, ..., dim_feedforward, dropout, activation)` with the reference's signature.

    precision: "bf16x3" (default: three-term split products on the matrix pipe, within 1e-4 of the fp32 reference), "fp32" (exact fp32 products) or
    "bf16" (throughput, no bar).
    """

    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048, dropout=0.1, activation="relu",
                 return_intermediate_dec=False, precision="bf16x3"):
        super().__init__()
        if activation != "relu":
            raise ValueError(f"SelfCrossTransformer: activation {activation!r} is not supported ({_LIMITS})")
        self.self_attn_layer0 = _Layer(d_model, nhead, dim_feedforward, dropout, cross=False)
        self.self_attn_layer1 = _Layer(d_model, nhead, dim_feedforward, dropout, cross=False)
        self.cross_attn_layer0 = _Layer(d_model, nhead, dim_feedforward, dropout, cross=True)
        self.cross_attn_layer1 = _Layer(d_model, nhead, dim_feedforward, dropout, cross=True)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.d_model, self.nhead, self.dim_feedforward = int(d_model), int(nhead), int(dim_feedforward)
        self.precision = check_precision(precision)
        self._cache_init()

    # ------------------------------------------------------------------ eager path (training / autograd)
    def _eager(self, v0, pos0, v1, pos1):
        v0, pos0, v1, pos1 = (t.transpose(0, 1) for t in (v0, pos0, v1, pos1))
        v0 = self.self_attn_layer0(v0, pos0, v0, pos0)
        v1 = self.self_attn_layer1(v1, pos1, v1, pos1)
        v0 = self.cross_attn_layer0(v0, pos0, v1, pos1)
        v1 = self.cross_attn_layer1(v1, pos1, v0, pos0)
        return v0.transpose(0, 1).contiguous(), v1.transpose(0, 1).contiguous()

    # ------------------------------------------------------------------ library path
    def _pack(self, device):
        lib = _lib.load()
        need = lib.nl_sct_packed_bytes(self.d_model, self.nhead, self.dim_feedforward)
        if need == 0:
            raise RuntimeError(f"SelfCrossTransformer: d_model {self.d_model}, nhead {self.nhead}, dim_feedforward {self.dim_feedforward} are not supported "
                               f"by the HIP kernels ({_LIMITS})")
        ps = list(self.parameters())   # registration order = state-dict order (the module has no buffers); cheaper per call than building the state dict
        if len(ps) != 52:
            raise RuntimeError("SelfCrossTransformer: expected the reference's 52 tensors")

        def pack(ts):
            arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            packed = torch.empty(need, dtype=torch.uint8, device=device)
            st = torch.cuda.current_stream(device).cuda_stream
            _lib.check(lib.nl_sct_pack_weights(self.d_model, self.nhead, self.dim_feedforward, arr, len(ts), packed.data_ptr(), need, st), "nl_sct_pack_weights")
            return packed
        return self._cached(device, ps, pack)

    def transform(self, v0, pos0, v1, pos1):
        """The library call: (out0 (B, N0, C), out1 (B, N1, C))."""
        ts = (v0, pos0, v1, pos1)
        require_device("SelfCrossTransformer", *ts)
        C = self.d_model
        if v0.dim() != 3 or v1.dim() != 3 or v0.shape[2] != C or v1.shape[2] != C or v0.shape[0] != v1.shape[0] or pos0.shape != v0.shape or pos1.shape != v1.shape:
            raise ValueError(f"SelfCrossTransformer: inputs must be (B, N0, {C}) and (B, N1, {C}) with position encodings of the same shapes")
        dev = v0.device
        B, N0, N1 = v0.shape[0], v0.shape[1], v1.shape[1]
        lib = _lib.load()
        with torch.cuda.device(dev):
            packed = self._pack(dev)   # raises for an unsupported configuration
            out0 = torch.empty((B, N0, C), dtype=torch.float32, device=dev)
            out1 = torch.empty((B, N1, C), dtype=torch.float32, device=dev)
            if B == 0:
                return out0, out1
            if N0 < 1 or N1 < 1:
                raise ValueError("SelfCrossTransformer: both sequences need at least one element")
            a = [t.detach().to(torch.float32).contiguous() for t in ts]   # the one copy of a non-contiguous input
            need = lib.nl_sct_workspace_bytes(B, N0, N1, C, self.dim_feedforward)
            if need == 0:
                raise RuntimeError(f"SelfCrossTransformer: B * max(N0, N1) = {B * max(N0, N1)} exceeds the kernels' limit of 2^24 rows")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.nl_sct_forward(packed.data_ptr(), C, self.nhead, self.dim_feedforward, _lib.PRECISIONS[self.precision], a[0].data_ptr(), a[1].data_ptr(),
                                          N0, a[2].data_ptr(), a[3].data_ptr(), N1, B, out0.data_ptr(), out1.data_ptr(), ws.data_ptr(), need, st), "nl_sct_forward")
        return out0, out1

    def forward(self, v0, pos_embed0, v1, pos_embed1):
        ts = (v0, pos_embed0, v1, pos_embed1)
        if self.training or (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
            return self._eager(*ts)
        return self.transform(*ts)
