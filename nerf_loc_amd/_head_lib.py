"""ctypes binding of libnerfloc_head.so (C-ABI in include/nerfloc_head.h): the head's device-side glue — match selection with a device count, the two position
encodings, the pose solver with device counts.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for `*_workspace_bytes` answers.  No fallback: a missing library or symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import stream

LIB_PATH = os.environ.get("NERFLOC_HEAD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_head.so")
HEADER = "nerfloc_head.h"
ABI_VERSION = 1  # the NLH_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
INFO_COUNT, INFO_TOTAL, INFO_OVERFLOW = 0, 1, 2   # nlh_select_matches: the words of `info`
SYMBOLS = _cabi.prototypes(HEADER, "nlh_")   # every symbol the header declares: (name, restype, argtypes)

_head = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _head
    if _head is None:
        _head = _cabi.bind(LIB_PATH, HEADER, "nlh_", "nlh_abi_version", "NLH_ABI_VERSION", ABI_VERSION, what="the head has no CPU fallback")
    return _head


def select_matches(match_j, cap, kps3d, kps2d, rows_a=None, rows_b=None):
    """nlh_select_matches on the current stream.  match_j (N) int32, kps3d (N, 3), kps2d (Mc, 2), rows_* (N, C) or None, all fp32 contiguous DEVICE tensors.
    -> dict(i_ids, j_ids, b_ids (cap) int64, mkps3d (cap, 3), mkps2d_c (cap, 2), out_a, out_b (cap, C) or None, info (4) int32)."""
    lib = load()
    dev = match_j.device
    N, Mc, cap = int(match_j.shape[0]), int(kps2d.shape[0]), int(cap)
    rows = [r for r in (rows_a, rows_b) if r is not None]
    Cc = int(rows[0].shape[1]) if rows else 0
    for t, shape in ((kps3d, (N, 3)), (kps2d, (Mc, 2))) + tuple((r, (N, Cc)) for r in rows):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"select_matches: expected a contiguous fp32 tensor of shape {shape} on {dev}")
    if match_j.dtype != torch.int32 or match_j.dim() != 1 or not match_j.is_contiguous() or cap < 1:
        raise ValueError("select_matches: match_j must be a contiguous (N) int32 tensor and cap >= 1")
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlh_select_workspace_bytes(N), dev, f"select_matches: N = {N} is outside 1 .. 2^20", ValueError)
        ids = torch.empty((3, cap), dtype=torch.int64, device=dev)
        mk3 = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        mk2 = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        oa = None if rows_a is None else torch.empty((cap, Cc), dtype=torch.float32, device=dev)
        ob = None if rows_b is None else torch.empty((cap, Cc), dtype=torch.float32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        ptr = _lib.ptr
        _lib.check(lib.nlh_select_matches(match_j.data_ptr(), N, cap, Mc, Cc, kps3d.data_ptr(), ptr(kps2d) if Mc else None, ptr(rows_a), ptr(rows_b), ids[0].data_ptr(),
                                          ids[1].data_ptr(), ids[2].data_ptr(), mk3.data_ptr(), mk2.data_ptr(), ptr(oa), ptr(ob), info.data_ptr(), ws.data_ptr(),
                                          ws.numel(), stream(dev)), "nlh_select_matches")
    return {"i_ids": ids[0], "j_ids": ids[1], "b_ids": ids[2], "mkps3d": mk3, "mkps2d_c": mk2, "out_a": oa, "out_b": ob, "info": info}


def pos_sine_grid(H, W, Cc, device):
    """nlh_pos_sine_grid: the (H, W, C) fp32 table on `device`."""
    lib = load()
    with torch.cuda.device(device):
        out = torch.empty((int(H), int(W), int(Cc)), dtype=torch.float32, device=device)
        _lib.check(lib.nlh_pos_sine_grid(int(H), int(W), int(Cc), out.data_ptr(), stream(device)), "nlh_pos_sine_grid")
    return out


def embed_points(x, L):
    """nlh_embed_points: x (..., D) on a HIP device -> (..., 2 D L) fp32."""
    lib = load()
    dev = x.device
    D = int(x.shape[-1])
    flat = x.detach().to(torch.float32).reshape(-1, D).contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((flat.shape[0], 2 * D * int(L)), dtype=torch.float32, device=dev)
        _lib.check(lib.nlh_embed_points(flat.data_ptr(), flat.shape[0], D, int(L), out.data_ptr(), stream(dev)), "nlh_embed_points")
    return out.reshape(*x.shape[:-1], 2 * D * int(L))
