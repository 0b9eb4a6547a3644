"""ctypes binding of libnerfloc_cnn.so (C-ABI in include/nerfloc_cnn.h): the per-frame visibility encoder DepthFusionNet.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for `*_workspace_bytes` answers.  No fallback: a missing library or symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, stream

LIB_PATH = os.environ.get("NERFLOC_CNN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_cnn.so")
HEADER = "nerfloc_cnn.h"
ABI_VERSION = 1  # the NLC_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
NUM_WEIGHTS, MIN_SIDE, MAX_VIEWS, MAX_PIXELS, LAUNCHES = (_D["NLC_DFNET_NUM_WEIGHTS"], _D["NLC_DFNET_MIN_SIDE"], _D["NLC_DFNET_MAX_VIEWS"],
                                                          _D["NLC_DFNET_MAX_PIXELS"], _D["NLC_DFNET_LAUNCHES"])


class NlcDfnetTaps(C.Structure):
    _fields_ = _cabi.struct_fields(HEADER)["nlc_dfnet_taps"]


STRUCTS = {"nlc_dfnet_taps": NlcDfnetTaps}
SYMBOLS = _cabi.prototypes(HEADER, "nlc_", STRUCTS)   # every symbol the header declares: (name, restype, argtypes)

_cnn = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _cnn
    if _cnn is None:
        _cnn = _cabi.bind(LIB_PATH, HEADER, "nlc_", "nlc_abi_version", "NLC_ABI_VERSION", ABI_VERSION, STRUCTS, what="the library path has no CPU fallback")
    return _cnn


def weight_names():
    """The 72 state-dict names (below `multiview_aggregator.depth_fusion.`) in the order nlc_dfnet_pack_weights takes them; needs no device."""
    lib = load()
    return [lib.nlc_dfnet_weight_name(i).decode() for i in range(lib.nlc_dfnet_num_weights())]


def supported(V, H, W) -> bool:
    """Whether (V, H, W) is inside the limits of nlc_dfnet_forward (the header's rule, restated for callers that choose a path without loading the library)."""
    return 1 <= V <= MAX_VIEWS and H >= MIN_SIDE and W >= MIN_SIDE and H % 16 == 0 and W % 16 == 0 and V * H * W <= MAX_PIXELS


def pack_weights(tensors):
    """nlc_dfnet_pack_weights on the current stream: the 72 dense fp32 device tensors in weight_names() order -> the packed image (uint8)."""
    lib = load()
    if len(tensors) != NUM_WEIGHTS:
        raise ValueError(f"pack_weights: expected {NUM_WEIGHTS} tensors")
    dev = tensors[0].device
    for t in tensors:
        if dense_f32(t, "pack_weights").device != dev:
            raise ValueError("pack_weights: the tensors lie on different devices")
    with torch.cuda.device(dev):
        need = lib.nlc_dfnet_packed_bytes()
        packed = torch.empty(need, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * NUM_WEIGHTS)(*[t.data_ptr() for t in tensors])
        _lib.check(lib.nlc_dfnet_pack_weights(ptrs, NUM_WEIGHTS, packed.data_ptr(), need, stream(dev)), "nlc_dfnet_pack_weights")
    return packed


def dfnet_forward(packed, cnn_in, taps=False, out=None):
    """nlc_dfnet_forward on the current stream.  cnn_in (V, 12, H, W) fp32 on a HIP device -> out (V, 32, H/4, W/4); taps=True: (out, x1, x2, x3)."""
    lib = load()
    if cnn_in.dim() != 4 or cnn_in.shape[1] != 12:
        raise ValueError("dfnet_forward: expected a (V, 12, H, W) tensor")
    dense_f32(cnn_in, "dfnet_forward")
    dev = cnn_in.device
    V, H, W = int(cnn_in.shape[0]), int(cnn_in.shape[2]), int(cnn_in.shape[3])
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlc_dfnet_workspace_bytes(V, H, W), dev, f"dfnet_forward: (V, H, W) = ({V}, {H}, {W}) is outside the limits", ValueError)
        if out is None:
            out = torch.empty((V, 32, H // 4, W // 4), dtype=torch.float32, device=dev)
        elif tuple(dense_f32(out, "dfnet_forward").shape) != (V, 32, H // 4, W // 4):
            raise ValueError("dfnet_forward: out must be (V, 32, H/4, W/4)")
        xs = [torch.empty((V, 32 << i, H >> (2 + i), W >> (2 + i)), dtype=torch.float32, device=dev) for i in range(3)] if taps else []
        tp = NlcDfnetTaps(*[x.data_ptr() for x in xs]) if taps else None
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.nlc_dfnet_forward(packed.data_ptr(), cnn_in.data_ptr(), V, H, W, out.data_ptr(), C.byref(tp) if taps else None, ws.data_ptr(), ws.numel(),
                                         st.cuda_stream), "nlc_dfnet_forward")
        ws.record_stream(st)
    return (out, *xs) if taps else out
