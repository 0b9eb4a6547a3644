"""ctypes binding of libnerfloc_counted.so (C-ABI in include/nerfloc_counted.h): the coarse matching stage with the number of 3-D points in device memory — the
SelfCrossTransformer with a counted sequence 0, one counted layer (the stage entry), and the mutual-nearest selection over the first n rows of a score matrix.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for the size queries' answers.  No fallback: a missing library or symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, ptr, stream

LIB_PATH = os.environ.get("NERFLOC_COUNTED_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_counted.so")
HEADER = "nerfloc_counted.h"
ABI_VERSION = 1  # the NLK_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
SYMBOLS = _cabi.prototypes(HEADER, "nlk_")   # every symbol the header declares, with its return and parameter types

_counted = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _counted
    if _counted is None:
        _counted = _cabi.bind(LIB_PATH, HEADER, "nlk_", "nlk_abi_version", "NLK_ABI_VERSION", ABI_VERSION, what="the counted matcher has no CPU fallback")
    return _counted


def device_count(n, what, device=None):
    """n, if it is what the library reads through a `const int32_t*`: a 0-d (or one-element) int32 tensor on a HIP device (`device`, if given).  A host integer or a
    CPU tensor raises: uploading it would hide a read-back at the caller's and freeze the value in a captured graph."""
    if not torch.is_tensor(n):
        raise TypeError(f"{what}: the count must be a 0-d int32 DEVICE tensor, not {type(n).__name__} (a host number would hide a read-back and defeat graph replay)")
    if not n.is_cuda or n.dtype != torch.int32 or n.numel() != 1 or (device is not None and n.device != device):
        raise ValueError(f"{what}: the count must be a 0-d int32 tensor on the inputs' HIP device")
    return n


def sct_forward_counted(packed, C_, nhead, F, precision, v0, pos0, v1, pos1, n0):
    """nlk_sct_forward_counted on the current stream: v0, pos0 (B, N0, C), v1, pos1 (B, N1, C) dense fp32; n0 a device count or None -> (out0, out1)."""
    lib = load()
    for t in (v0, pos0, v1, pos1):
        dense_f32(t, "sct_forward_counted")
    dev = v0.device
    B, N0, N1 = int(v0.shape[0]), int(v0.shape[1]), int(v1.shape[1])
    if n0 is not None:
        device_count(n0, "sct_forward_counted", dev)
    with torch.cuda.device(dev):
        out0 = torch.empty((B, N0, C_), dtype=torch.float32, device=dev)
        out1 = torch.empty((B, N1, C_), dtype=torch.float32, device=dev)
        if B == 0:
            return out0, out1
        ws = _lib.workspace(lib.nlk_sct_workspace_bytes(B, N0, N1, C_, F), dev, f"sct_forward_counted: (B, N0, N1) = ({B}, {N0}, {N1}) is outside the limits", ValueError)
        _lib.check(lib.nlk_sct_forward_counted(packed.data_ptr(), C_, nhead, F, precision, v0.data_ptr(), pos0.data_ptr(), N0, ptr(n0), v1.data_ptr(), pos1.data_ptr(),
                                               N1, B, out0.data_ptr(), out1.data_ptr(), ws.data_ptr(), ws.numel(), stream(dev)), "nlk_sct_forward_counted")
    return out0, out1


def sct_layer_counted(packed, C_, nhead, F, layer, precision, x, x_pos, mem, mem_pos, nk):
    """nlk_sct_layer_counted: x, x_pos (B, Nq, C); mem, mem_pos (B, Nk, C), or None for a self layer; nk a device count or None -> out (B, Nq, C)."""
    lib = load()
    for t in (x, x_pos) + (() if mem is None else (mem, mem_pos)):
        dense_f32(t, "sct_layer_counted")
    dev = x.device
    B, Nq = int(x.shape[0]), int(x.shape[1])
    Nk = Nq if mem is None else int(mem.shape[1])
    if nk is not None:
        device_count(nk, "sct_layer_counted", dev)
    with torch.cuda.device(dev):
        out = torch.empty_like(x)
        ws = _lib.workspace(lib.nlk_sct_workspace_bytes(B, Nq, Nk, C_, F), dev, "sct_layer_counted: outside the limits", ValueError)
        _lib.check(lib.nlk_sct_layer_counted(packed.data_ptr(), C_, nhead, F, int(layer), precision, x.data_ptr(), x_pos.data_ptr(), Nq, ptr(mem), ptr(mem_pos), Nk,
                                             ptr(nk), B, out.data_ptr(), ws.data_ptr(), ws.numel(), stream(dev)), "nlk_sct_layer_counted")
    return out


def s2d_select_counted(scores, n, thr):
    """nlk_s2d_select_counted: scores (N, M) dense fp32 >= 0, n a device count or None -> (match_j (N) int32, match_score (N) fp32)."""
    lib = load()
    dense_f32(scores, "s2d_select_counted")
    if scores.dim() != 2:
        raise ValueError("s2d_select_counted: scores must be (N, M)")
    dev = scores.device
    N, M = int(scores.shape[0]), int(scores.shape[1])
    if n is not None:
        device_count(n, "s2d_select_counted", dev)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlk_s2d_select_workspace_bytes(N, M), dev, f"s2d_select_counted: (N, M) = ({N}, {M}) is outside the limits", ValueError)
        match_j = torch.empty(N, dtype=torch.int32, device=dev)
        match_s = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.check(lib.nlk_s2d_select_counted(scores.data_ptr(), N, M, ptr(n), C.c_float(float(thr)), match_j.data_ptr(), match_s.data_ptr(), ws.data_ptr(), ws.numel(),
                                              stream(dev)), "nlk_s2d_select_counted")
    return match_j, match_s
