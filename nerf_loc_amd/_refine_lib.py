"""ctypes binding of libnerfloc_refine.so (C-ABI in include/nerfloc_refine.h): pose refinement around the renderer's forward / backward pair — the se(3) maps,
the rays of a pose, the bilinear target, the masked loss, the pose gradient and Adam.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes.  No fallback: a missing library or symbol raises.  Nothing here synchronises or reads a result back: every function
enqueues on torch's current stream and returns device tensors.  The loop functions (`pose_rays`, `loss`, `step`) take the caller's buffers and return nothing:
they are what a captured refinement step replays.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, ptr, stream

LIB_PATH = os.environ.get("NERFLOC_REFINE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_refine.so")
HEADER = "nerfloc_refine.h"
ABI_VERSION = 1  # the NLR_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
POSE_F32, POSE_F64, LAYOUT_NCHW, LAYOUT_NHWC = _D["NLR_POSE_F32"], _D["NLR_POSE_F64"], _D["NLR_LAYOUT_NCHW"], _D["NLR_LAYOUT_NHWC"]
MAX_POSES, MAX_RAYS, MAX_CHANNELS, STATE_DOUBLES = _D["NLR_MAX_POSES"], _D["NLR_MAX_RAYS"], _D["NLR_MAX_CHANNELS"], _D["NLR_STATE_DOUBLES"]
# the words of one pose's record in the state block (nerfloc_refine.h: THE STATE BLOCK)
S_PARAMS, S_M, S_V, S_GRAD, S_LOSS_INIT, S_LOSS_LAST, S_POSE0, S_T, S_NAN = slice(0, 6), slice(6, 12), slice(12, 18), slice(18, 24), 24, 25, slice(26, 42), 42, 43
SYMBOLS = _cabi.prototypes(HEADER, "nlr_")   # every symbol the header declares, with its return and parameter types

_refine = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _refine
    if _refine is None:
        _refine = _cabi.bind(LIB_PATH, HEADER, "nlr_", "nlr_abi_version", "NLR_ABI_VERSION", ABI_VERSION, what="the library path has no CPU fallback")
    return _refine


def _dense(t, dtype, what):
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor on a HIP device")
    return t


def _f64_rows(t, shape, what):
    if tuple(t.shape[1:]) != shape:
        raise ValueError(f"{what}: expected (N, {', '.join(map(str, shape))})")
    return _dense(t, torch.float64, what)


def se3_exp(p):
    """nlr_se3_exp: (N, 6) fp64 -> (N, 4, 4) fp64."""
    lib, dev = load(), _f64_rows(p, (6,), "se3_exp").device
    with torch.cuda.device(dev):
        T = torch.empty((p.shape[0], 4, 4), dtype=torch.float64, device=dev)
        _lib.check(lib.nlr_se3_exp(p.data_ptr(), int(p.shape[0]), T.data_ptr(), stream(dev)), "nlr_se3_exp")
    return T


def se3_exp_backward(p, G):
    """nlr_se3_exp_backward: p (N, 6), G (N, 4, 4) fp64 -> d sum(G * exp(p)) / d p (N, 6) fp64."""
    lib, dev = load(), _f64_rows(p, (6,), "se3_exp_backward").device
    if _f64_rows(G, (4, 4), "se3_exp_backward").shape[0] != p.shape[0]:
        raise ValueError("se3_exp_backward: p and G differ in N")
    with torch.cuda.device(dev):
        g = torch.empty_like(p)
        _lib.check(lib.nlr_se3_exp_backward(p.data_ptr(), G.data_ptr(), int(p.shape[0]), g.data_ptr(), stream(dev)), "nlr_se3_exp_backward")
    return g


def se3_log(T):
    """nlr_se3_log: (N, 4, 4) fp64 -> (N, 6) fp64."""
    lib, dev = load(), _f64_rows(T, (4, 4), "se3_log").device
    with torch.cuda.device(dev):
        p = torch.empty((T.shape[0], 6), dtype=torch.float64, device=dev)
        _lib.check(lib.nlr_se3_log(T.data_ptr(), int(T.shape[0]), p.data_ptr(), stream(dev)), "nlr_se3_log")
    return p


def state_bytes(B: int) -> int:
    return int(load().nlr_state_bytes(int(B)))


def new_state(B: int, device) -> torch.Tensor:
    """An uninitialised state block: (B, STATE_DOUBLES) fp64 (the counter and the latch are int64 words: `state.view(torch.int64)[:, S_T]`)."""
    if state_bytes(B) == 0:
        raise ValueError(f"refine: 1 <= B <= {MAX_POSES} poses per call")
    return torch.empty((int(B), STATE_DOUBLES), dtype=torch.float64, device=device)


def init(poses, state):
    """nlr_init: poses (B, 4, 4) fp32 / fp64, read as they lie -> state."""
    lib = load()
    if not poses.is_cuda or poses.dtype not in (torch.float32, torch.float64) or not poses.is_contiguous() or tuple(poses.shape) != (state.shape[0], 4, 4):
        raise ValueError("refine.init: poses must be contiguous fp32 or fp64 (B, 4, 4) on a HIP device")
    dev = poses.device
    with torch.cuda.device(dev):
        _lib.check(lib.nlr_init(poses.data_ptr(), POSE_F64 if poses.dtype == torch.float64 else POSE_F32, int(state.shape[0]), state.data_ptr(), stream(dev)), "nlr_init")


def pose_rays(state, K, uv, Rp, pose32, rays_o, rays_d, centres):
    """nlr_pose_rays into the caller's buffers: rays_o, rays_d, centres (B Rp, 3) fp32, pose32 (B, 4, 4) fp32 or None."""
    lib, dev, B = load(), state.device, int(state.shape[0])
    dense_f32(K, "pose_rays"), dense_f32(uv, "pose_rays")
    for t in (rays_o, rays_d, centres):
        if dense_f32(t, "pose_rays").numel() != B * int(Rp) * 3:
            raise ValueError("pose_rays: the ray buffers hold (B Rp, 3) values")
    if K.numel() != 9 or uv.numel() != 2 * int(Rp) or (pose32 is not None and dense_f32(pose32, "pose_rays").numel() != 16 * B):
        raise ValueError("pose_rays: K (3, 3), uv (Rp, 2), pose32 (B, 4, 4)")
    with torch.cuda.device(dev):
        _lib.check(lib.nlr_pose_rays(state.data_ptr(), K.data_ptr(), uv.data_ptr(), B, int(Rp), ptr(pose32), rays_o.data_ptr(), rays_d.data_ptr(), centres.data_ptr(),
                                     stream(dev)), "nlr_pose_rays")


def sample_target(fmap, H, W, uv):
    """nlr_sample_target: fmap (C, h, w) or (1, C, h, w) fp32 — contiguous, or channels_last (read as it lies) — -> (Rp, C) fp32: the bilinear resize to (H, W) at uv."""
    lib = load()
    if fmap.dim() == 4 and fmap.shape[0] == 1:
        layout = LAYOUT_NCHW if fmap.is_contiguous() else LAYOUT_NHWC if fmap.is_contiguous(memory_format=torch.channels_last) else None
        fmap = fmap[0]
    elif fmap.dim() == 3:
        layout = LAYOUT_NCHW if fmap.is_contiguous() else LAYOUT_NHWC if fmap.permute(1, 2, 0).is_contiguous() else None
    else:
        raise ValueError("sample_target: one map, (C, h, w) or (1, C, h, w)")
    if layout is None or fmap.dtype != torch.float32 or not fmap.is_cuda:
        raise ValueError("sample_target: the map must be fp32 on a HIP device, contiguous or channels_last")
    dense_f32(uv, "sample_target")
    dev, (Cc, h, w), Rp = fmap.device, fmap.shape, int(uv.shape[0])
    with torch.cuda.device(dev):
        out = torch.empty((Rp, Cc), dtype=torch.float32, device=dev)
        _lib.check(lib.nlr_sample_target(fmap.data_ptr(), layout, int(Cc), int(h), int(w), int(H), int(W), uv.data_ptr(), Rp, out.data_ptr(), stream(dev)),
                   "nlr_sample_target")
    return out


def loss(out, mask, target, B, Rp, g_out, row_loss):
    """nlr_loss into the caller's buffers: out (B Rp, C) fp32, mask (B Rp) uint8 / bool, target (Rp, C) fp32 -> g_out (B Rp, C) fp32, row_loss (B Rp) fp64."""
    lib, dev = load(), out.device
    dense_f32(out, "loss"), dense_f32(target, "loss"), dense_f32(g_out, "loss"), _dense(row_loss, torch.float64, "loss")
    Cc = int(target.shape[-1])
    if mask.dtype not in (torch.uint8, torch.bool) or not mask.is_contiguous() or mask.numel() != B * Rp or out.numel() != B * Rp * Cc or g_out.numel() != out.numel() \
            or target.numel() != Rp * Cc or row_loss.numel() != B * Rp:
        raise ValueError("loss: out / g_out (B Rp, C), mask (B Rp) uint8, target (Rp, C), row_loss (B Rp)")
    with torch.cuda.device(dev):
        _lib.check(lib.nlr_loss(out.data_ptr(), mask.data_ptr(), target.data_ptr(), int(B), int(Rp), Cc, g_out.data_ptr(), row_loss.data_ptr(), stream(dev)), "nlr_loss")


def step(state, row_loss, g_rays_o, g_rays_d, g_centres, K, uv, Rp, C_, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """nlr_step: one refinement step of every pose of the state, in place."""
    lib, dev, B = load(), state.device, int(state.shape[0])
    _dense(row_loss, torch.float64, "step"), dense_f32(K, "step"), dense_f32(uv, "step")
    for t in (g_rays_o, g_rays_d, g_centres):
        if dense_f32(t, "step").numel() != B * int(Rp) * 3:
            raise ValueError("step: the ray cotangents hold (B Rp, 3) values")
    if row_loss.numel() != B * int(Rp) or uv.numel() != 2 * int(Rp) or K.numel() != 9:
        raise ValueError("step: row_loss (B Rp), uv (Rp, 2), K (3, 3)")
    with torch.cuda.device(dev):
        _lib.check(lib.nlr_step(state.data_ptr(), row_loss.data_ptr(), g_rays_o.data_ptr(), g_rays_d.data_ptr(), g_centres.data_ptr(), K.data_ptr(), uv.data_ptr(), B,
                                int(Rp), int(C_), float(lr), float(beta1), float(beta2), float(eps), stream(dev)), "nlr_step")


def finish(state):
    """nlr_finish -> T_c2w (B, 4, 4) fp64, T_c2w32 (B, 4, 4) fp32, info (B, 4) fp64 = (loss_init, loss_last, accepted, nan)."""
    lib, dev, B = load(), state.device, int(state.shape[0])
    with torch.cuda.device(dev):
        T64 = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
        T32 = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        info = torch.empty((B, 4), dtype=torch.float64, device=dev)
        _lib.check(lib.nlr_finish(state.data_ptr(), B, T64.data_ptr(), T32.data_ptr(), info.data_ptr(), stream(dev)), "nlr_finish")
    return T64, T32, info
