"""ctypes binding of libnerfloc_backbone.so (C-ABI in include/nerfloc_backbone.h): the 2-D backbone, ResNet-50 to layer2 + FPN.

Built by the same `make` as libnerfloc_render.so (`_lib.build()`), bound from its header by the same layer (`_cabi.bind`), and it speaks `_lib`'s conventions:
`_lib.check` for the NL_* status codes, `_lib.workspace` for `*_workspace_bytes` answers.  No fallback: a missing library or symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _cabi, _lib
from ._cabi import dense_f32, stream

LIB_PATH = os.environ.get("NERFLOC_BACKBONE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnerfloc_backbone.so")
HEADER = "nerfloc_backbone.h"
ABI_VERSION = 1  # the NLB_ABI_VERSION these wrappers were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)
NUM_WEIGHTS, MIN_SIDE, MAX_VIEWS, MAX_PIXELS, LAUNCHES = (_D["NLB_BACKBONE_NUM_WEIGHTS"], _D["NLB_BACKBONE_MIN_SIDE"], _D["NLB_BACKBONE_MAX_VIEWS"],
                                                          _D["NLB_BACKBONE_MAX_PIXELS"], _D["NLB_BACKBONE_LAUNCHES"])
PRECISIONS = {"fp32": _D["NLB_PRECISION_FP32"], "bf16x3": _D["NLB_PRECISION_BF16X3"]}
LAYOUTS = {"nchw": _D["NLB_LAYOUT_NCHW"], "channels_last": _D["NLB_LAYOUT_CHANNELS_LAST"]}
FPN_DIMS = (64, 128, 192, 256)


class NlbBackboneTaps(C.Structure):
    _fields_ = _cabi.struct_fields(HEADER)["nlb_backbone_taps"]


STRUCTS = {"nlb_backbone_taps": NlbBackboneTaps}
SYMBOLS = _cabi.prototypes(HEADER, "nlb_", STRUCTS)   # every symbol the header declares: (name, restype, argtypes)

_bb = None


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _bb
    if _bb is None:
        _bb = _cabi.bind(LIB_PATH, HEADER, "nlb_", "nlb_abi_version", "NLB_ABI_VERSION", ABI_VERSION, STRUCTS, what="the library path has no CPU fallback")
    return _bb


def weight_names():
    """The 124 state-dict names in the order nlb_backbone_pack_weights takes them; needs no device."""
    lib = load()
    return [lib.nlb_backbone_weight_name(i).decode() for i in range(NUM_WEIGHTS)]


def half_up(n):
    """The side of a map after a stride-2 stage: (n - 1) / 2 + 1."""
    return (n - 1) // 2 + 1


def plane_sizes(H, W):
    """((h1, w1), (h2, w2), (h3, w3)): the planes of conv1, layer1 and layer2."""
    h1, w1 = half_up(H), half_up(W)
    h2, w2 = half_up(h1), half_up(w1)
    return (h1, w1), (h2, w2), (half_up(h2), half_up(w2))


def supported(V, H, W, fpn_dim) -> bool:
    """Whether the call is inside the limits of nlb_backbone_forward (the header's rule, restated for callers that choose a path without loading the library)."""
    return 1 <= V <= MAX_VIEWS and H >= MIN_SIDE and W >= MIN_SIDE and V * H * W <= MAX_PIXELS and fpn_dim in FPN_DIMS


def pack_weights(tensors, fpn_dim):
    """nlb_backbone_pack_weights on the current stream: the 124 dense fp32 device tensors in weight_names() order -> the packed image (uint8)."""
    lib = load()
    if len(tensors) != NUM_WEIGHTS:
        raise ValueError(f"pack_weights: expected {NUM_WEIGHTS} tensors")
    dev = tensors[0].device
    for t in tensors:
        if dense_f32(t, "pack_weights").device != dev:
            raise ValueError("pack_weights: the tensors lie on different devices")
    with torch.cuda.device(dev):
        need = lib.nlb_backbone_packed_bytes(fpn_dim)
        if need == 0:
            raise ValueError(f"pack_weights: fpn_dim {fpn_dim} is not one of {FPN_DIMS}")
        packed = torch.empty(need, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * NUM_WEIGHTS)(*[t.data_ptr() for t in tensors])
        _lib.check(lib.nlb_backbone_pack_weights(ptrs, NUM_WEIGHTS, fpn_dim, packed.data_ptr(), need, stream(dev)), "nlb_backbone_pack_weights")
    return packed


def backbone_forward(packed, imgs, fpn_dim, precision="fp32", layout="channels_last", taps=False):
    """nlb_backbone_forward on the current stream.  imgs (V, 3, H, W) fp32 on a HIP device -> (conv1, layer1, layer2); taps=True: also the raw layer1 and layer2
    maps.  The FPN maps have the logical shape (V, fpn_dim, h, w); with layout "channels_last" their memory is NHWC (permute(0, 2, 3, 1) is contiguous)."""
    lib = load()
    if precision not in PRECISIONS:
        raise ValueError(f"backbone_forward: unknown precision {precision!r}")
    if layout not in LAYOUTS:
        raise ValueError(f"backbone_forward: unknown layout {layout!r}")
    if imgs.dim() != 4 or imgs.shape[1] != 3:
        raise ValueError("backbone_forward: expected a (V, 3, H, W) tensor")
    dense_f32(imgs, "backbone_forward")
    dev = imgs.device
    V, H, W = int(imgs.shape[0]), int(imgs.shape[2]), int(imgs.shape[3])
    (h1, w1), (h2, w2), (h3, w3) = plane_sizes(H, W)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nlb_backbone_workspace_bytes(V, H, W, fpn_dim), dev,
                            f"backbone_forward: (V, H, W, fpn_dim) = ({V}, {H}, {W}, {fpn_dim}) is outside the limits", ValueError)
        c1 = torch.empty((V, 64, h1, w1), dtype=torch.float32, device=dev)
        if layout == "channels_last":
            p1 = torch.empty((V, h2, w2, fpn_dim), dtype=torch.float32, device=dev)
            p2 = torch.empty((V, h3, w3, fpn_dim), dtype=torch.float32, device=dev)
        else:
            p1 = torch.empty((V, fpn_dim, h2, w2), dtype=torch.float32, device=dev)
            p2 = torch.empty((V, fpn_dim, h3, w3), dtype=torch.float32, device=dev)
        xs = [torch.empty((V, 256, h2, w2), dtype=torch.float32, device=dev), torch.empty((V, 512, h3, w3), dtype=torch.float32, device=dev)] if taps else []
        tp = NlbBackboneTaps(*[x.data_ptr() for x in xs]) if taps else None
        st = torch.cuda.current_stream(dev)
        _lib.check(lib.nlb_backbone_forward(packed.data_ptr(), imgs.data_ptr(), V, H, W, fpn_dim, PRECISIONS[precision], LAYOUTS[layout], c1.data_ptr(),
                                            p1.data_ptr(), p2.data_ptr(), C.byref(tp) if taps else None, ws.data_ptr(), ws.numel(), st.cuda_stream),
                   "nlb_backbone_forward")
        ws.record_stream(st)
    if layout == "channels_last":
        p1, p2 = p1.permute(0, 3, 1, 2), p2.permute(0, 3, 1, 2)
    return (c1, p1, p2, *xs) if taps else (c1, p1, p2)
