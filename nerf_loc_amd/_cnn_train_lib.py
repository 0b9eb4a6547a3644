"""ctypes binding of libnerfloc_cnn_train.so (C-ABI in include/nerfloc_cnn_train.h): DepthFusionNet for training — the forward that keeps its state, the backward
that writes the 72 parameter gradients, and the stage entry points (one convolution's gradients, one InstanceNorm's, the bilinear x 2's).

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for the size queries' answers.  No fallback: a missing library or symbol raises.  The weight names and
the limits are libnerfloc_cnn.so's (`_cnn_lib`).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _cnn_lib, _lib
from ._cabi import dense_f32, ptr, stream

LIB_PATH = os.environ.get("NERFLOC_CNN_TRAIN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_cnn_train.so")
HEADER = "nerfloc_cnn_train.h"
ABI_VERSION = 1  # the NLCT_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
FORWARD_LAUNCHES, BACKWARD_LAUNCHES = _D["NLCT_FORWARD_LAUNCHES"], _D["NLCT_BACKWARD_LAUNCHES"]
NUM_WEIGHTS = _cnn_lib.NUM_WEIGHTS
ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
SYMBOLS = _cabi.prototypes(HEADER, "nlct_")   # every symbol the header declares, with its return and parameter types

_cnnt = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _cnnt
    if _cnnt is None:
        _cnnt = _cabi.bind(LIB_PATH, HEADER, "nlct_", "nlct_abi_version", "NLCT_ABI_VERSION", ABI_VERSION, what="the library path has no CPU fallback")
    return _cnnt


def pack_weights(tensors):
    """nlct_dfnet_pack_weights on the current stream: the 72 dense fp32 device tensors in `_cnn_lib.weight_names()` order -> the training image (uint8)."""
    lib = load()
    if len(tensors) != NUM_WEIGHTS:
        raise ValueError(f"pack_weights: expected {NUM_WEIGHTS} tensors")
    dev = tensors[0].device
    for t in tensors:
        if dense_f32(t, "pack_weights").device != dev:
            raise ValueError("pack_weights: the tensors lie on different devices")
    with torch.cuda.device(dev):
        need = lib.nlct_dfnet_packed_bytes()
        packed = torch.empty(need, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * NUM_WEIGHTS)(*[t.data_ptr() for t in tensors])
        _lib.check(lib.nlct_dfnet_pack_weights(ptrs, NUM_WEIGHTS, packed.data_ptr(), need, stream(dev)), "nlct_dfnet_pack_weights")
    return packed


def _shape(cnn_in, what):
    if cnn_in.dim() != 4 or cnn_in.shape[1] != 12:
        raise ValueError(f"{what}: expected a (V, 12, H, W) tensor")
    dense_f32(cnn_in, what)
    return int(cnn_in.shape[0]), int(cnn_in.shape[2]), int(cnn_in.shape[3])


def dfnet_forward_train(packed, cnn_in, state=None):
    """nlct_dfnet_forward_train on the current stream -> (out (V, 32, H/4, W/4), state (uint8)); `state`: the caller's buffer of nlct_dfnet_state_bytes bytes."""
    lib = load()
    V, H, W = _shape(cnn_in, "dfnet_forward_train")
    dev = cnn_in.device
    with torch.cuda.device(dev):
        need = lib.nlct_dfnet_state_bytes(V, H, W)
        if state is None:
            state = _lib.workspace(need, dev, f"dfnet_forward_train: (V, H, W) = ({V}, {H}, {W}) is outside the limits", ValueError)
        elif state.dtype != torch.uint8 or state.device != dev or not state.is_contiguous() or state.numel() < need or need == 0:
            raise ValueError("dfnet_forward_train: state must be a contiguous uint8 tensor of nlct_dfnet_state_bytes(V, H, W) bytes on cnn_in's device")
        out = torch.empty((V, 32, H // 4, W // 4), dtype=torch.float32, device=dev)
        _lib.check(lib.nlct_dfnet_forward_train(packed.data_ptr(), cnn_in.data_ptr(), V, H, W, out.data_ptr(), state.data_ptr(), state.numel(), stream(dev)),
                   "nlct_dfnet_forward_train")
    return out, state


def dfnet_backward(packed, cnn_in, state, g_out, shapes, wanted=None):
    """nlct_dfnet_backward on the current stream.  shapes: the 72 parameter shapes in weight order; wanted: 72 flags (None = all) -> a list of 72 fp32 tensors,
    None where not wanted."""
    lib = load()
    V, H, W = _shape(cnn_in, "dfnet_backward")
    if tuple(dense_f32(g_out, "dfnet_backward").shape) != (V, 32, H // 4, W // 4):
        raise ValueError("dfnet_backward: g_out must be (V, 32, H/4, W/4)")
    if len(shapes) != NUM_WEIGHTS or (wanted is not None and len(wanted) != NUM_WEIGHTS):
        raise ValueError(f"dfnet_backward: expected {NUM_WEIGHTS} shapes and flags")
    dev = cnn_in.device
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlct_dfnet_backward_workspace_bytes(V, H, W), dev, f"dfnet_backward: (V, H, W) = ({V}, {H}, {W}) is outside the limits", ValueError)
        grads = [torch.empty(tuple(s), dtype=torch.float32, device=dev) if wanted is None or wanted[i] else None for i, s in enumerate(shapes)]
        ptrs = (C.c_void_p * NUM_WEIGHTS)(*[ptr(g) for g in grads])
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.nlct_dfnet_backward(packed.data_ptr(), cnn_in.data_ptr(), V, H, W, state.data_ptr(), g_out.data_ptr(), ptrs, ws.data_ptr(), ws.numel(),
                                           st.cuda_stream), "nlct_dfnet_backward")
        ws.record_stream(st)
    return grads


def conv_backward(x0, x1, w, g_y, stride, want_x=True, want_w=True):
    """nlct_conv_backward: x0 (V, C0, h, w), x1 (V, C1, h, w) or None, w (cout, C0 + C1, ks, ks), g_y (V, cout, ho, wo) -> (g_x0, g_x1, g_w), None where not wanted."""
    lib = load()
    for t in (x0, w, g_y) + (() if x1 is None else (x1,)):
        dense_f32(t, "conv_backward")
    dev = x0.device
    V, C0, hin, win = (int(v) for v in x0.shape)
    C1 = 0 if x1 is None else int(x1.shape[1])
    cout, ks = int(w.shape[0]), int(w.shape[2])
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlct_conv_backward_workspace_bytes(V, C0, C1, cout, hin, win, ks, int(stride)), dev, "conv_backward: outside the limits", ValueError)
        g_x0 = torch.empty_like(x0) if want_x else None
        g_x1 = torch.empty_like(x1) if want_x and x1 is not None else None
        g_w = torch.empty_like(w) if want_w else None
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.nlct_conv_backward(x0.data_ptr(), C0, ptr(x1), C1, w.data_ptr(), g_y.data_ptr(), V, cout, hin, win, ks, int(stride), ptr(g_x0), ptr(g_x1),
                                          ptr(g_w), ws.data_ptr(), ws.numel(), st.cuda_stream), "nlct_conv_backward")
        ws.record_stream(st)
    return g_x0, g_x1, g_w


def instnorm_backward(x, nrm, y, act, g_y):
    """nlct_instnorm_backward: x, g_y (V, C, n), nrm (V, C, 4), y (V, C, n) or None -> (g_x, g_gamma, g_beta)."""
    lib = load()
    for t in (x, nrm, g_y) + (() if y is None else (y,)):
        dense_f32(t, "instnorm_backward")
    dev = x.device
    V, Cc, n = (int(v) for v in x.shape)
    with torch.cuda.device(dev):
        ws = torch.empty(max(8 * V * Cc, 256), dtype=torch.uint8, device=dev)
        g_x, g_gamma, g_beta = torch.empty_like(x), torch.empty(Cc, dtype=torch.float32, device=dev), torch.empty(Cc, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.nlct_instnorm_backward(x.data_ptr(), nrm.data_ptr(), ptr(y), int(act), g_y.data_ptr(), V, Cc, n, g_x.data_ptr(), g_gamma.data_ptr(),
                                              g_beta.data_ptr(), ws.data_ptr(), ws.numel(), st.cuda_stream), "nlct_instnorm_backward")
        ws.record_stream(st)
    return g_x, g_gamma, g_beta


def up2_backward(g_y):
    """nlct_up2_backward: g_y (P, 2 h, 2 w) -> g_x (P, h, w)."""
    lib = load()
    dense_f32(g_y, "up2_backward")
    P, h, w = int(g_y.shape[0]), int(g_y.shape[1]) // 2, int(g_y.shape[2]) // 2
    dev = g_y.device
    with torch.cuda.device(dev):
        g_x = torch.empty((P, h, w), dtype=torch.float32, device=dev)
        _lib.check(lib.nlct_up2_backward(g_y.data_ptr(), P, h, w, g_x.data_ptr(), stream(dev)), "nlct_up2_backward")
    return g_x
