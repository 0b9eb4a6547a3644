"""ctypes binding of libnerfloc_app.so (C-ABI in include/nerfloc_app.h): appearance adaptation — channel statistics, the adaptation MLP, FiLM and its gradients.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for `*_workspace_bytes` answers.  No fallback: a missing library or symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, stream

LIB_PATH = os.environ.get("NERFLOC_APP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_app.so")
HEADER = "nerfloc_app.h"
ABI_VERSION = 1  # the NLA_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
LAYOUT_NCHW, LAYOUT_NHWC = _D["NLA_LAYOUT_NCHW"], _D["NLA_LAYOUT_NHWC"]
FILM_CLIP01 = _D["NLA_FILM_CLIP01"]
HIDDEN = _D["NLA_ADAPT_HIDDEN"]
SYMBOLS = _cabi.prototypes(HEADER, "nla_")   # every symbol the header declares: (name, restype, argtypes)

_app = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _app
    if _app is None:
        _app = _cabi.bind(LIB_PATH, HEADER, "nla_", "nla_abi_version", "NLA_ABI_VERSION", ABI_VERSION, what="the library path has no CPU fallback")
    return _app


def channel_stats(x, layout=None):
    """nla_channel_stats on the current stream.  x (B, C, H, W) fp32 on a HIP device, dense as NCHW or as channels_last (used as it lies; `layout` forces the
    reading of an ambiguous tensor) -> (B, 2 C): means, then unbiased standard deviations."""
    lib = load()
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("channel_stats: expected a (B, C, H, W) fp32 tensor on a HIP device")
    if layout is None:
        layout = LAYOUT_NCHW if x.is_contiguous() else LAYOUT_NHWC
    if not (x.is_contiguous() if layout == LAYOUT_NCHW else x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("channel_stats: the tensor is not dense in the stated layout")
    dev = x.device
    B, Cc, HW = int(x.shape[0]), int(x.shape[1]), int(x.shape[2] * x.shape[3])
    with torch.cuda.device(dev):
        out = torch.empty((B, 2 * Cc), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        ws = _lib.workspace(lib.nla_channel_stats_workspace_bytes(B, Cc, HW, layout), dev, f"channel_stats: C = {Cc} or H W = {HW} is outside the limits", ValueError)
        _lib.check(lib.nla_channel_stats(x.data_ptr(), B, Cc, HW, layout, out.data_ptr(), ws.data_ptr(), ws.numel(), stream(dev)), "nla_channel_stats")
    return out


def adapt_code(emb, target, weights):
    """nla_adapt_code: emb (V, E), target (E) or (1, E), weights: the six tensors of the MLP in state-dict order -> code (V, 2 C)."""
    lib = load()
    dev = emb.device
    V, E = int(emb.shape[0]), int(emb.shape[1])
    C2 = int(weights[4].shape[0])
    shapes = ((HIDDEN, E), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (C2, HIDDEN), (C2,))
    for w, shape in zip(weights, shapes):
        if tuple(w.shape) != shape or w.device != dev:
            raise ValueError(f"adapt_code: expected a weight of shape {shape} on {dev}")
        dense_f32(w, "adapt_code")
    if target.numel() != E or C2 % 2:
        raise ValueError("adapt_code: target must hold E values and the last layer 2 C rows")
    dense_f32(emb, "adapt_code"), dense_f32(target, "adapt_code")
    with torch.cuda.device(dev):
        code = torch.empty((V, C2), dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * 6)(*[w.data_ptr() for w in weights])
        _lib.check(lib.nla_adapt_code(emb.data_ptr(), target.data_ptr(), ptrs, V, E, C2 // 2, code.data_ptr(), stream(dev)), "nla_adapt_code")
    return code


def film(x, code, clip=False, out=None):
    """nla_film: x (V, ..., C) contiguous, code (V, 2 C) -> y of x's shape (out=x: in place)."""
    lib = load()
    dev = x.device
    V, Cc = int(x.shape[0]), int(x.shape[-1])
    dense_f32(x, "film"), dense_f32(code, "film")
    if tuple(code.shape) != (V, 2 * Cc):
        raise ValueError("film: code must be (V, 2 C)")
    HW = x.numel() // max(V * Cc, 1)
    with torch.cuda.device(dev):
        y = torch.empty_like(x) if out is None else dense_f32(out, "film")
        if x.numel():
            _lib.check(lib.nla_film(x.data_ptr(), code.data_ptr(), V, HW, Cc, FILM_CLIP01 if clip else 0, y.data_ptr(), stream(dev)), "nla_film")
    return y


def film_backward(x, code, g_y, clip=False, want_x=True, want_code=True, g_x_out=None):
    """nla_film_backward -> (g_x or None, g_code or None); g_x_out=g_y writes g_x in place."""
    lib = load()
    dev = x.device
    V, Cc = int(x.shape[0]), int(x.shape[-1])
    dense_f32(x, "film_backward"), dense_f32(code, "film_backward"), dense_f32(g_y, "film_backward")
    if g_y.shape != x.shape or tuple(code.shape) != (V, 2 * Cc):
        raise ValueError("film_backward: g_y must have x's shape and code must be (V, 2 C)")
    HW = x.numel() // max(V * Cc, 1)
    with torch.cuda.device(dev):
        g_x = (torch.empty_like(x) if g_x_out is None else dense_f32(g_x_out, "film_backward")) if want_x else None
        g_code = torch.empty((V, 2 * Cc), dtype=torch.float32, device=dev) if want_code else None
        if not x.numel():
            return g_x, (g_code.zero_() if want_code else None)
        ws = _lib.workspace(lib.nla_film_backward_workspace_bytes(V, HW, Cc), dev, "film_backward: the shape is outside the limits", ValueError) if want_code else None
        _lib.check(lib.nla_film_backward(x.data_ptr(), code.data_ptr(), g_y.data_ptr(), V, HW, Cc, FILM_CLIP01 if clip else 0, _lib.ptr(g_x), _lib.ptr(g_code),
                                         _lib.ptr(ws), ws.numel() if want_code else 0, stream(dev)), "nla_film_backward")
    return g_x, g_code
