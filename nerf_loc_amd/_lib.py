"""ctypes binding of libnerfloc_render.so (C-ABI in include/nerfloc_render.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent this module
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from . import _cabi
from ._cabi import dense_f32, ptr, stream, workspace  # noqa: F401  -- the call helpers, under the names the package's modules use

_HERE = os.path.dirname(os.path.abspath(__file__))
# NERFLOC_LIB: developer override used for same-box A/B timing of two builds of the library
LIB_PATH = os.environ.get("NERFLOC_LIB") or os.path.join(_HERE, "csrc", "libnerfloc_render.so")

NL_OK = 0
NL_ERR_BAD_ARG, NL_ERR_UNSUPPORTED, NL_ERR_WORKSPACE, NL_ERR_HIP, NL_ERR_NO_DEVICE = -1, -2, -3, -4, -5
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_F16MX = 0, 1, 2, 3
# "f16mx" (round 4): BF16X3 everywhere except the fused neural-point kernel of render_rays, which multiplies as fp16 hi.hi + two MX cross terms (FP6 elements since round 5, FP8 in round 4)
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16": PREC_BF16, "f16mx": PREC_F16MX}
PRECISION_NAMES = {PREC_F32: "fp32", PREC_BF16X3: "bf16x3", PREC_BF16: "bf16", PREC_F16MX: "f16mx"}
HEADER = "nerfloc_render.h"
ABI_VERSION = 13  # the NL_ABI_VERSION the wrappers of this package were written against (load() holds it against the header's and the library's)
_D = _cabi.defines(HEADER)   # the header's #defines are read, not copied
MAX_VIEWS = _D["NL_MAX_VIEWS"]
RENDER_NO_SIDE_STREAM = _D["NL_RENDER_NO_SIDE_STREAM"]    # nl_render_opts.flags
RENDER_PRECISION_GUARD = _D["NL_RENDER_PRECISION_GUARD"]  # nl_render_opts.flags (ABI 7): the library checks the conditioning indicator after the batch and re-renders it in a more exact mode if needed
GUARD_LOGIT_LIMIT = {k[21:].lower(): v for k, v in _D.items() if k.startswith("NL_GUARD_LOGIT_LIMIT_")}      # {"f16mx": 50.0, "bf16x3": 500.0}
GUARD_DENSITY_LIMIT = {k[23:].lower(): v for k, v in _D.items() if k.startswith("NL_GUARD_DENSITY_LIMIT_")}  # {"f16mx": 32.0}: the guard's second indicator, the largest density of the frame's guarded batches; bf16x3 has no such limit
DIAG_COUNT = _D["NL_DIAG_COUNT"]
FINE_BACKWARD_MAX_M = _D["NL_FINE_BACKWARD_MAX_M"]  # above it the fine matcher's modules train on the eager path


class NlConfig(C.Structure):
    _fields_ = [("W", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("precision", C.c_int32)]


class NlFrameDesc(C.Structure):
    _fields_ = [
        ("V", C.c_int32), ("H", C.c_int32), ("Wimg", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("vis_h", C.c_int32), ("vis_w", C.c_int32),
        ("near_", C.c_float), ("far_", C.c_float),
        ("images", C.c_void_p), ("featmaps", C.c_void_p), ("vis_featmaps", C.c_void_p),
        ("proj_ibr", C.c_void_p), ("proj_neuray", C.c_void_p), ("cam_centers", C.c_void_p),
        ("M", C.c_int64),
        ("sp_xyz", C.c_void_p), ("sp_feature", C.c_void_p), ("sp_confidence", C.c_void_p), ("sp_direction", C.c_void_p),
    ]


class NlRenderOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "rgb", "depth", "weights", "mask", "depth_uncertainty", "feat",
        "sigma", "feature_agg", "mv_feature_agg", "geo", "knn_idx", "knn_d2")]


class NlRenderOpts(C.Structure):
    _fields_ = [("early_term_eps", C.c_float), ("flags", C.c_uint32), ("ray_centers", C.c_void_p), ("reserved", C.c_int32 * 4)]


class NlRenderJob(C.Structure):   # include/nerfloc_render.h: nl_render_job
    _fields_ = [("frame", C.c_void_p), ("query_center", C.c_void_p), ("rays_o", C.c_void_p), ("rays_d", C.c_void_p), ("z_vals", C.c_void_p), ("R", C.c_int64),
                ("out", C.POINTER(NlRenderOut)), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("opts", C.POINTER(NlRenderOpts))]


class NlTrainGrads(C.Structure):
    _fields_ = [("weights", C.POINTER(C.c_void_p)), ("support_feature", C.c_void_p), ("feat_maps", C.c_void_p), ("vis_featmaps", C.c_void_p),
                ("blend_feat_maps", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("reserved", C.c_int32 * 4)]


class NlRenderCotangents(C.Structure):
    _fields_ = [("g_rgb", C.c_void_p), ("g_depth", C.c_void_p), ("g_depth_uncertainty", C.c_void_p), ("g_feat", C.c_void_p), ("g_weights", C.c_void_p),
                ("knn_idx", C.c_void_p), ("knn_d2", C.c_void_p), ("reserved", C.c_void_p * 1)]


class NlBetaHead(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("beta_min", C.c_float), ("beta", C.c_void_p), ("g_beta", C.c_void_p), ("g_weight", C.c_void_p),
                ("g_bias", C.c_void_p)]


STRUCTS = {"nl_config": NlConfig, "nl_frame_desc": NlFrameDesc, "nl_render_out": NlRenderOut, "nl_render_opts": NlRenderOpts, "nl_render_job": NlRenderJob,
           "nl_train_grads": NlTrainGrads, "nl_render_cotangents": NlRenderCotangents, "nl_beta_head": NlBetaHead}
SYMBOLS = _cabi.prototypes(HEADER, "nl_", STRUCTS)   # every symbol the header declares: (name, restype, argtypes)

_lib = None


def build(verbose: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libnerfloc_render.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    if verbose:
        print(res.stdout[-2000:])
    return LIB_PATH


def load() -> C.CDLL:
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        _lib = _cabi.bind(LIB_PATH, HEADER, "nl_", "nl_abi_version", "NL_ABI_VERSION", ABI_VERSION, STRUCTS, "there is no CPU fallback for the renderer")
    return _lib


def check(status: int, what: str = "") -> None:
    if status != NL_OK:
        msg = load().nl_strerror(status).decode()
        raise RuntimeError(f"libnerfloc_render {what}: {msg} ({status})")


def weight_names():
    lib = load()
    return [lib.nl_weight_name(i).decode() for i in range(lib.nl_num_weights())]
