"""Drop-in for the reference's `SelfCrossTransformer` (models/COTR/transformer.py:17-64, used twice by matcher.py: coarse :68-72 and fine :120-124).

Eval mode on a HIP device is ONE library call (nl_sct_forward, csrc/sct.hip): four post-norm layers, each a projection kernel, a flash-style attention kernel that
never writes an Nq x Nk tensor, and a row-chain kernel (out_proj, residual, LayerNorm, FFN, residual, LayerNorm) whose hidden rows stay on chip.  Training mode, or
an input that requires grad while grad is enabled, runs the same four layers in eager PyTorch through the same sub-modules by default.  Eval mode on CPU tensors is
refused: no CPU fallback.

`hip_training = True` (opt-in, default False) replaces that eager stretch by the library's training step whenever NO dropout is in effect (the constructor's
dropout == 0, or eval mode): one autograd Function around nl_sct_forward_train / nl_sct_backward (csrc/sct_bwd.hip), which keeps O(rows x C) of state, never a
heads x Nq x Nk tensor, and gives the same bits on every call.  Training mode with dropout > 0 (the reference's Matcher constructs both transformers with
dropout = 0.1) stays eager unless `hip_dropout` is set too.

`hip_dropout = True` (opt-in, default False; needs `hip_training`) takes the library's step in training mode with 0 < dropout < 1 as well: nl_sct_forward_train_dropout
/ nl_sct_backward_dropout drop at the reference's four sites per layer (attention probabilities, out_proj's output, the ReLU'd hidden rows, linear2's output) inside
the kernels.  The masks are a counter-based function of (seed, p, layer, site, element) — Philox4x32-10, 16-bit thresholds, scale 1 / (actual keep probability);
csrc/sct_drop.h, restated in tests/sct_dropout_ref.py — recomputed in the backward: nothing per element is kept.  They are NOT torch's masks: same distribution,
other bits.  One seed per forward: `dropout_seed` if it is an int (tests, reproducible steps: every forward then drops the same elements), else a draw from torch's
default CPU generator, which follows torch.manual_seed and needs no device synchronisation.  The autograd Function keeps (p, seed) for its backward.  The seed is a
host value: a forward captured in a HIP graph replays one seed.  dropout >= 1, CPU tensors, shapes outside the limits: eager, as before.  Eval mode is unaffected.

The sub-modules carry the reference's names (`self_attn_layer{0,1}.self_attn / linear1 / linear2 / norm1 / norm2`, `cross_attn_layer{0,1}.multihead_attn /
linear1 / linear2 / norm1 / norm2 / norm3`), so `matcher.coarse_transformer.*` and `matcher.fine_transformer.*` of a NeRF-Loc checkpoint load with strict=True.
The decoder layers' norm1 is constructed and never applied, as in the reference.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _counted_lib, _lib
from ._packing import PackedCache, check_precision, new_train_cache, require_device

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


_UNUSED_PARAMS = (32, 33, 46, 47)   # state-dict indices of the cross layers' norm1 pair: constructed, never applied, no gradient


class _TrainStep(torch.autograd.Function):
    """nl_sct_forward_train / nl_sct_backward around the module's four layers; the 52 parameters are inputs so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, mod, p, seed, v0, pos0, v1, pos1, *params):
        lib = _lib.load()
        dev = v0.device
        C, Fh = mod.d_model, mod.dim_feedforward
        B, N0, N1 = v0.shape[0], v0.shape[1], v1.shape[1]
        with torch.cuda.device(dev):
            packed, tpacked = mod._pack(dev), mod._pack_train(dev)
            a = [t.detach().to(torch.float32).contiguous() for t in (v0, pos0, v1, pos1)]
            out0 = torch.empty((B, N0, C), dtype=torch.float32, device=dev)
            out1 = torch.empty((B, N1, C), dtype=torch.float32, device=dev)
            sb, wb = lib.nl_sct_train_state_bytes(B, N0, N1, C, Fh), lib.nl_sct_workspace_bytes(B, N0, N1, C, Fh)
            state = torch.empty(sb, dtype=torch.uint8, device=dev)
            ws = torch.empty(wb, dtype=torch.uint8, device=dev)
            st = _lib.stream(dev)
            args = (packed.data_ptr(), C, mod.nhead, Fh, _lib.PRECISIONS[mod.precision], a[0].data_ptr(), a[1].data_ptr(), N0, a[2].data_ptr(), a[3].data_ptr(), N1, B,
                    out0.data_ptr(), out1.data_ptr(), state.data_ptr(), sb, ws.data_ptr(), wb)
            if p > 0:
                _lib.check(lib.nl_sct_forward_train_dropout(*args, p, seed, st), "nl_sct_forward_train_dropout")
            else:
                _lib.check(lib.nl_sct_forward_train(*args, st), "nl_sct_forward_train")
        ctx.drop = (p, seed)
        ctx.mod, ctx.images, ctx.inputs, ctx.state, ctx.dims = mod, (packed, tpacked), a, state, (B, N0, N1)
        ctx.in_dtypes = [t.dtype for t in (v0, pos0, v1, pos1)]
        ctx.param_meta = [(p.shape, p.dtype) for p in params]
        ctx.set_materialize_grads(False)
        return out0, out1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g0, g1):
        lib = _lib.load()
        mod, a, (B, N0, N1) = ctx.mod, ctx.inputs, ctx.dims
        dev = a[0].device
        C, Fh = mod.d_model, mod.dim_feedforward
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            g0, g1 = (None if g is None else g.to(torch.float32).contiguous() for g in (g0, g1))
            gin = [torch.empty_like(a[i]) if need[3 + i] else None for i in range(4)]
            gpar = [torch.empty(shape, dtype=torch.float32, device=dev) if need[7 + i] and i not in _UNUSED_PARAMS else None
                    for i, (shape, _) in enumerate(ctx.param_meta)]
            ptr = _lib.ptr
            arr = (ctypes.c_void_p * len(gpar))(*[ptr(t) for t in gpar])
            wb = lib.nl_sct_backward_workspace_bytes(B, N0, N1, C, Fh)
            ws = torch.empty(wb, dtype=torch.uint8, device=dev)
            st = _lib.stream(dev)
            args = (ctx.images[0].data_ptr(), ctx.images[1].data_ptr(), C, mod.nhead, Fh, _lib.PRECISIONS[mod.precision], a[0].data_ptr(), a[1].data_ptr(), N0,
                    a[2].data_ptr(), a[3].data_ptr(), N1, B, ctx.state.data_ptr(), ctx.state.numel(), ptr(g0), ptr(g1), ptr(gin[0]), ptr(gin[1]), ptr(gin[2]),
                    ptr(gin[3]), arr, len(gpar), ws.data_ptr(), wb)
            p, seed = ctx.drop
            if p > 0:
                _lib.check(lib.nl_sct_backward_dropout(*args, p, seed, st), "nl_sct_backward_dropout")
            else:
                _lib.check(lib.nl_sct_backward(*args, st), "nl_sct_backward")
        gin = [g if g is None else g.to(dt) for g, dt in zip(gin, ctx.in_dtypes)]
        gpar = [g if g is None else g.to(dt) for g, (_, dt) in zip(gpar, ctx.param_meta)]
        return (None, None, None, *gin, *gpar)


class SelfCrossTransformer(nn.Module, PackedCache):
    """`SelfCrossTransformer(d_model, nhead, ..., dim_feedforward, dropout, activation)` with the reference's signature.

    precision: "bf16x3" (default: three-term split products on the matrix pipe, within 1e-4 of the fp32 reference), "fp32" (exact fp32 products) or
    "bf16" (throughput, no bar).
    hip_training (attribute, default False): take the library's training step instead of eager autograd where it applies (see the module docstring).
    hip_dropout (attribute, default False): with hip_training, also in training mode with 0 < dropout < 1 — dropout inside the kernels, with the library's masks.
    dropout_seed (attribute, default None): an int fixes the mask seed of every forward; None draws one per forward from torch's default CPU generator.
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
        self.dropout = float(dropout)
        self.hip_training = False
        self.hip_dropout = False
        self.dropout_seed = None
        self.precision = check_precision(precision)
        self._cache_init()
        self._train_cache = new_train_cache()

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
            st = _lib.stream(device)
            _lib.check(lib.nl_sct_pack_weights(self.d_model, self.nhead, self.dim_feedforward, arr, len(ts), packed.data_ptr(), need, st), "nl_sct_pack_weights")
            return packed
        return self._cached(device, ps, pack)

    def _pack_train(self, device):
        """The training image (the transposed weights nl_sct_backward multiplies by), cached like the inference image."""
        lib = _lib.load()
        need = lib.nl_sct_train_packed_bytes(self.d_model, self.nhead, self.dim_feedforward)
        ps = list(self.parameters())

        def pack(ts):
            arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            packed = torch.empty(need, dtype=torch.uint8, device=device)
            st = _lib.stream(device)
            _lib.check(lib.nl_sct_pack_weights_train(self.d_model, self.nhead, self.dim_feedforward, arr, len(ts), packed.data_ptr(), need, st),
                       "nl_sct_pack_weights_train")
            return packed
        return self._train_cache._cached(device, ps, pack)

    def _library_training_applies(self, ts):
        """hip_training, HIP tensors, a gradient wanted, no dropout in effect (or hip_dropout and dropout < 1), and a shape inside the library's limits (decided at
        forward time)."""
        if not self.hip_training or not all(t.is_cuda for t in ts):
            return False
        grad = torch.is_grad_enabled() and (any(t.requires_grad for t in ts) or any(p.requires_grad for p in self.parameters()))
        if not (self.training or grad) or (self.training and self.dropout > 0 and not (self.hip_dropout and self.dropout < 1)):
            return False
        v0, pos0, v1, pos1 = ts
        C = self.d_model
        if v0.dim() != 3 or v1.dim() != 3 or v0.shape[2] != C or v1.shape[2] != C or v0.shape[0] != v1.shape[0] or pos0.shape != v0.shape or pos1.shape != v1.shape:
            return False
        if v0.shape[0] < 1 or v0.shape[1] < 1 or v1.shape[1] < 1 or len(list(self.parameters())) != 52:
            return False
        return _lib.load().nl_sct_train_state_bytes(v0.shape[0], v0.shape[1], v1.shape[1], C, self.dim_feedforward) != 0 and self.nhead == 8

    def transform(self, v0, pos0, v1, pos1, n0=None):
        """The library call: (out0 (B, N0, C), out1 (B, N1, C)).  n0 (default None: every row exists) is a 0-d int32 DEVICE tensor: only the first n0 rows of
        sequence 0 exist — nlk_sct_forward_counted (libnerfloc_counted.so); out0[:, :n0] and out1 then carry the bits of the call on v0[:, :n0].  The rows behind
        n0 must be finite.  A host integer or a CPU tensor raises."""
        ts = (v0, pos0, v1, pos1)
        require_device("SelfCrossTransformer", *ts)
        C = self.d_model
        if v0.dim() != 3 or v1.dim() != 3 or v0.shape[2] != C or v1.shape[2] != C or v0.shape[0] != v1.shape[0] or pos0.shape != v0.shape or pos1.shape != v1.shape:
            raise ValueError(f"SelfCrossTransformer: inputs must be (B, N0, {C}) and (B, N1, {C}) with position encodings of the same shapes")
        dev = v0.device
        B, N0, N1 = v0.shape[0], v0.shape[1], v1.shape[1]
        lib = _lib.load()
        if n0 is not None:
            _counted_lib.device_count(n0, "SelfCrossTransformer.transform", dev)
            if N0 < 1 or N1 < 1:
                raise ValueError("SelfCrossTransformer: both sequences need at least one element")
            with torch.cuda.device(dev):
                a = [t.detach().to(torch.float32).contiguous() for t in ts]
                return _counted_lib.sct_forward_counted(self._pack(dev), C, self.nhead, self.dim_feedforward, _lib.PRECISIONS[self.precision], *a, n0)
        with torch.cuda.device(dev):
            packed = self._pack(dev)   # raises for an unsupported configuration
            out0 = torch.empty((B, N0, C), dtype=torch.float32, device=dev)
            out1 = torch.empty((B, N1, C), dtype=torch.float32, device=dev)
            if B == 0:
                return out0, out1
            if N0 < 1 or N1 < 1:
                raise ValueError("SelfCrossTransformer: both sequences need at least one element")
            a = [t.detach().to(torch.float32).contiguous() for t in ts]   # the one copy of a non-contiguous input
            ws = _lib.workspace(lib.nl_sct_workspace_bytes(B, N0, N1, C, self.dim_feedforward), dev,
                                f"SelfCrossTransformer: B * max(N0, N1) = {B * max(N0, N1)} exceeds the kernels' limit of 2^24 rows")
            st = _lib.stream(dev)
            _lib.check(lib.nl_sct_forward(packed.data_ptr(), C, self.nhead, self.dim_feedforward, _lib.PRECISIONS[self.precision], a[0].data_ptr(), a[1].data_ptr(),
                                          N0, a[2].data_ptr(), a[3].data_ptr(), N1, B, out0.data_ptr(), out1.data_ptr(), ws.data_ptr(), ws.numel(), st), "nl_sct_forward")
        return out0, out1

    def forward(self, v0, pos_embed0, v1, pos_embed1):
        ts = (v0, pos_embed0, v1, pos_embed1)
        if self._library_training_applies(ts):
            p, seed = 0.0, 0
            if self.training and self.dropout > 0:   # hip_dropout: one seed per forward, a host value
                p = self.dropout
                seed = self.dropout_seed if isinstance(self.dropout_seed, int) else int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
                seed &= 2 ** 64 - 1
            return _TrainStep.apply(self, p, seed, *ts, *self.parameters())
        if self.training or (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
            return self._eager(*ts)
        return self.transform(*ts)
