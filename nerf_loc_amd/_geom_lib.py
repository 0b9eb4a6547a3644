"""ctypes binding of libnerfloc_geom.so (C-ABI in include/nerfloc_geom.h): keypoint geometry — visibility, 3D-2D pairs, the dense loss target, the cell grid.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for `*_workspace_bytes` answers.  No fallback: a missing library or symbol raises.  Nothing here
synchronises or reads a result back: every function returns device tensors, counts included.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, stream

LIB_PATH = os.environ.get("NERFLOC_GEOM_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_geom.so")
HEADER = "nerfloc_geom.h"
ABI_VERSION = 1  # the NLG_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
POSE_F32, POSE_F64, DEPTH_MAP, DEPTH_POINTS = _D["NLG_POSE_F32"], _D["NLG_POSE_F64"], _D["NLG_DEPTH_MAP"], _D["NLG_DEPTH_POINTS"]
TARGET_F32, TARGET_I64 = _D["NLG_TARGET_F32"], _D["NLG_TARGET_I64"]
MAX_POINTS, MAX_VIEWS, CHUNK, MIN_POSITIVES = _D["NLG_MAX_POINTS"], _D["NLG_MAX_VIEWS"], _D["NLG_CHUNK"], _D["NLG_MIN_POSITIVES"]
SYMBOLS = _cabi.prototypes(HEADER, "nlg_")   # every symbol the header declares: (name, restype, argtypes)

_geom = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _geom
    if _geom is None:
        _geom = _cabi.bind(LIB_PATH, HEADER, "nlg_", "nlg_abi_version", "NLG_ABI_VERSION", ABI_VERSION, what="the library path has no CPU fallback")
    return _geom


def _pose_flag(pose, shape, what):
    """The flag of a dense fp32 / fp64 pose tensor on a HIP device whose trailing shape is `shape`."""
    if not pose.is_cuda or pose.dtype not in (torch.float32, torch.float64) or not pose.is_contiguous() or tuple(pose.shape[-len(shape):]) != shape:
        raise ValueError(f"{what}: poses must be contiguous fp32 or fp64 {shape} on a HIP device")
    return POSE_F64 if pose.dtype == torch.float64 else POSE_F32


def _points(pts, what):
    if pts.dim() != 2 or pts.shape[1] != 3 or not 1 <= pts.shape[0] <= MAX_POINTS:
        raise ValueError(f"{what}: points must be (N, 3) with 1 <= N <= {MAX_POINTS}")
    return dense_f32(pts, what)


def select_visible(pts, poses, K, H, W, cap=None):
    """nlg_select_visible on the current stream.  pts (N, 3) fp32, poses (V, 4, 4) fp32 / fp64, K (3, 3) fp32 -> mask (N) bool, idx (cap) int64, info (4) int32."""
    lib = load()
    _points(pts, "select_visible"), dense_f32(K, "select_visible")
    if poses.dim() != 3 or not 1 <= poses.shape[0] <= MAX_VIEWS or tuple(K.shape) != (3, 3):
        raise ValueError(f"select_visible: poses must be (V, 4, 4) with 1 <= V <= {MAX_VIEWS} and K (3, 3)")
    flags = _pose_flag(poses, (4, 4), "select_visible")
    dev, N = pts.device, int(pts.shape[0])
    cap = N if cap is None else int(cap)
    with torch.cuda.device(dev):
        mask = torch.empty(N, dtype=torch.bool, device=dev)
        idx = torch.empty(cap, dtype=torch.int64, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.nlg_select_visible_workspace_bytes(N), dev, "select_visible: N is outside the limits", ValueError)
        _lib.check(lib.nlg_select_visible(pts.data_ptr(), N, poses.data_ptr(), int(poses.shape[0]), K.data_ptr(), int(H), int(W), flags, cap, mask.data_ptr(),
                                          idx.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), stream(dev)), "nlg_select_visible")
    return mask, idx, info


def build_pairs(pts, pose, K, H, W, stride, thr, depth, depth_points=False, cap=None):
    """nlg_build_pairs -> dict(proj (N, 2), z (N), valid, pos (N) bool, gt_j (N) int32, pairs (2, cap) int64, info (4) int32).  depth: the (H, W) map, or
    with depth_points the (N) array."""
    lib = load()
    _points(pts, "build_pairs"), dense_f32(K, "build_pairs"), dense_f32(depth, "build_pairs")
    dev, N = pts.device, int(pts.shape[0])
    if tuple(K.shape) != (3, 3) or tuple(depth.shape) != ((N,) if depth_points else (int(H), int(W))):
        raise ValueError("build_pairs: K must be (3, 3) and depth (H, W), or (N) with depth_points")
    flags = _pose_flag(pose, (4, 4), "build_pairs") | (DEPTH_POINTS if depth_points else DEPTH_MAP)
    if pose.dim() != 2:
        raise ValueError("build_pairs: one (4, 4) pose")
    cap = N if cap is None else int(cap)
    with torch.cuda.device(dev):
        out = {"proj": torch.empty((N, 2), dtype=torch.float32, device=dev), "z": torch.empty(N, dtype=torch.float32, device=dev),
               "valid": torch.empty(N, dtype=torch.bool, device=dev), "pos": torch.empty(N, dtype=torch.bool, device=dev),
               "gt_j": torch.empty(N, dtype=torch.int32, device=dev), "pairs": torch.empty((2, cap), dtype=torch.int64, device=dev),
               "info": torch.empty(4, dtype=torch.int32, device=dev)}
        ws = _lib.workspace(lib.nlg_build_pairs_workspace_bytes(N), dev, "build_pairs: N is outside the limits", ValueError)
        _lib.check(lib.nlg_build_pairs(pts.data_ptr(), N, pose.data_ptr(), K.data_ptr(), int(H), int(W), int(stride), float(thr), depth.data_ptr(), flags, cap,
                                       out["proj"].data_ptr(), out["z"].data_ptr(), out["valid"].data_ptr(), out["pos"].data_ptr(), out["gt_j"].data_ptr(),
                                       out["pairs"].data_ptr(), out["info"].data_ptr(), ws.data_ptr(), ws.numel(), stream(dev)), "nlg_build_pairs")
    return out


def conf_target(gt_j, M, dtype=torch.float32, rows=None):
    """nlg_conf_target -> the (N, M) target, or with rows = (begin, end) the (end - begin, M) slice of it (nothing else is allocated)."""
    lib = load()
    if gt_j.dtype != torch.int32 or not gt_j.is_cuda or not gt_j.is_contiguous() or gt_j.dim() != 1:
        raise ValueError("conf_target: gt_j must be a contiguous (N) int32 tensor on a HIP device")
    if dtype not in (torch.float32, torch.int64):
        raise ValueError("conf_target: the target is fp32 or int64")
    dev, N, M = gt_j.device, int(gt_j.shape[0]), int(M)
    begin, end = (0, N) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= begin <= end <= N or N < 1 or M < 1:
        raise ValueError("conf_target: 0 <= begin <= end <= N, N >= 1 and M >= 1")
    with torch.cuda.device(dev):
        out = torch.empty((end - begin, M), dtype=dtype, device=dev)
        if end == begin:
            return out
        base =out.data_ptr() - begin * M * out.element_size()   # the address element (0, 0) would have: only the rows of the range are touched
        _lib.check(lib.nlg_conf_target(gt_j.data_ptr(), N, M, TARGET_F32 if dtype == torch.float32 else TARGET_I64, begin, end, base, stream(dev)),
                   "nlg_conf_target")
    return out


def cell_grid(Hc, Wc, scale=1.0, device="cuda"):
    """nlg_cell_grid -> (Hc Wc, 2) fp32: (x, y) * scale."""
    lib = load()
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = torch.empty((int(Hc) * int(Wc), 2), dtype=torch.float32, device=dev)
        _lib.check(lib.nlg_cell_grid(int(Hc), int(Wc), float(scale), out.data_ptr(), stream(dev)), "nlg_cell_grid")
    return out
