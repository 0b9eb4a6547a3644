"""The fifth library's boundary and the per-frame encoder's contract, without a GPU: header against binding against symbol table, the weight names against the
module's state dict, the header's arithmetic (tests/dfnet_ref.py) against the reference's fixtures, and the opt-in switch of DepthFusionNet on the CPU."""
import ctypes as ct
import functools
import os
import re
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from nerf_loc_amd import _app_lib, _cabi, _cnn_lib, _geom_lib, _head_lib, _lib
from nerf_loc_amd.depth_fusion import DepthFusionNet
from tests import dfnet_cases as dc
from tests import dfnet_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerfloc_cnn.h")
RESTATED = 1e-12   # fp64 restatement against the reference's fp64
GUARD = 1.25e-5    # a tensor whose recorded fp32 error is above this is ill-conditioned on that recipe (tests/test_gpu_dfnet.py)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"dfnet_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


def build_module(name, device="cpu"):
    _, w = dc.build(name)
    m = DepthFusionNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.to(device)


# ------------------------------------------------------------------------------------------ the fifth library's boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlc_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_cnn_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_cnn_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 7 and "nlc_dfnet_forward" in declared and "nlc_dfnet_pack_weights" in declared
    assert sorted(n for n, _, _ in _cnn_lib.SYMBOLS) == declared
    assert _exported(_cnn_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no symbol of another library
    lib = _cnn_lib.load()
    hdr = open(HEADER).read()
    assert lib.nlc_abi_version() == _cnn_lib.ABI_VERSION == int(re.search(r"#define\s+NLC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    assert _cnn_lib.NUM_WEIGHTS == lib.nlc_dfnet_num_weights() == 72
    # signatures: read from the header, no hand-written argtypes
    sig = {n: (r, a) for n, r, a in _cnn_lib.SYMBOLS}
    V, I, Z = ct.c_void_p, ct.c_int, ct.c_size_t
    assert sig["nlc_dfnet_forward"] == (I, [V, V, I, I, I, V, ct.POINTER(_cnn_lib.NlcDfnetTaps), V, Z, V])
    assert sig["nlc_dfnet_pack_weights"] == (I, [ct.POINTER(V), I, V, Z, V])
    assert sig["nlc_dfnet_weight_name"] == (ct.c_char_p, [I]) and sig["nlc_dfnet_workspace_bytes"] == (Z, [I, I, I])
    # the one struct: three pointers, nothing else
    assert _cabi.struct_fields("nerfloc_cnn.h") == {"nlc_dfnet_taps": [("x1", V), ("x2", V), ("x3", V)]}
    assert ct.sizeof(_cnn_lib.NlcDfnetTaps) == 24


def test_the_other_four_libraries_export_no_cnn_symbol():
    for other in (_lib, _head_lib, _app_lib, _geom_lib):
        assert not [n for n in _exported(other.LIB_PATH) if n.startswith("nlc_")]


def test_weight_names_are_the_state_dict_keys_in_order():
    names = _cnn_lib.weight_names()   # a host-only query
    assert names == list(DepthFusionNet().state_dict().keys()) and len(names) == 72
    lib = _cnn_lib.load()
    assert lib.nlc_dfnet_weight_name(-1) is None and lib.nlc_dfnet_weight_name(72) is None
    assert lib.nlc_dfnet_packed_bytes() % 256 == 0


def test_limits_and_refusals_without_a_device():
    lib = _cnn_lib.load()
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 255) // 256 * 256   # a HOST address no call below may read: every call here is refused before a launch
    for V, H, W in ((1, 32, 32), (2, 32, 48), (3, 48, 80), (10, 256, 336), (64, 1024, 1024)):
        assert lib.nlc_dfnet_workspace_bytes(V, H, W) > 0 and _cnn_lib.supported(V, H, W)
    for V, H, W in ((0, 32, 32), (65, 32, 32), (1, 16, 32), (1, 32, 16), (1, 40, 64), (1, 36, 48), (1, 56, 64), (-1, 32, 32), (64, 1024, 1040)):
        assert lib.nlc_dfnet_workspace_bytes(V, H, W) == 0 and not _cnn_lib.supported(V, H, W)
    need = lib.nlc_dfnet_workspace_bytes(1, 32, 32)
    call = lambda packed, x, V, H, W, out, taps, ws, n: lib.nlc_dfnet_forward(packed, x, V, H, W, out, taps, ws, n, None)
    assert call(p, p, 1, 40, 64, p, None, p, 1 << 30) == _lib.NL_ERR_UNSUPPORTED
    assert call(p, p, 0, 32, 32, p, None, p, 1 << 30) == _lib.NL_ERR_UNSUPPORTED
    assert call(None, p, 1, 32, 32, p, None, p, need) == _lib.NL_ERR_BAD_ARG and call(p, None, 1, 32, 32, p, None, p, need) == _lib.NL_ERR_BAD_ARG
    assert call(p, p, 1, 32, 32, None, None, p, need) == _lib.NL_ERR_BAD_ARG and call(p, p + 4, 1, 32, 32, p, None, p, need) == _lib.NL_ERR_BAD_ARG
    W = _lib.NL_ERR_WORKSPACE
    assert call(p, p, 1, 32, 32, p, None, None, need) == W and call(p, p, 1, 32, 32, p, None, p, need - 1) == W and call(p, p, 1, 32, 32, p, None, p + 16, need) == W
    ptrs = (ct.c_void_p * 72)(*([p] * 72))
    nb = lib.nlc_dfnet_packed_bytes()
    assert lib.nlc_dfnet_pack_weights(ptrs, 71, p, nb, None) == _lib.NL_ERR_BAD_ARG and lib.nlc_dfnet_pack_weights(None, 72, p, nb, None) == _lib.NL_ERR_BAD_ARG
    assert lib.nlc_dfnet_pack_weights(ptrs, 72, p, nb - 1, None) == W and lib.nlc_dfnet_pack_weights(ptrs, 72, p + 16, nb, None) == W
    ptrs[5] = None
    assert lib.nlc_dfnet_pack_weights(ptrs, 72, p, nb, None) == _lib.NL_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------ the header's arithmetic against the reference
@pytest.mark.parametrize("name", list(dc.CASES))
def test_restated_encoder_equals_the_reference(name):
    """Every tensor at 1e-12, with one exception: `out` of `const`.  There every input plane has zero variance, the InstanceNorms divide rounding noise by
    sqrt(eps), and the reference's own fp32 run misses its fp64 run by 2.4 on that tensor: two fp64 programs agree to 1e-6 on it, not to 1e-12."""
    x, w = dc.build(name)
    g, r = golden(name), dr.dfnet_forward(x, w)
    for k in dc.TENSORS:
        print(name, k, rel(r[k], g[k]), "recorded fp32_dev", float(g["fp32_dev_" + k]))
        assert np.isfinite(r[k]).all()
        if name == "const" and k == "out":
            assert float(g["fp32_dev_out"]) > 1.0
            continue
        assert rel(r[k], g[k]) <= RESTATED, (name, k)


def test_fixture_shapes_and_recorded_errors():
    for name, (V, H, W, _, _) in dc.CASES.items():
        g = golden(name)
        assert g["out"].shape == (V, 32, H // 4, W // 4) and g["x1"].shape == (V, 32, H // 4, W // 4)
        assert g["x2"].shape == (V, 64, H // 8, W // 8) and g["x3"].shape == (V, 128, H // 16, W // 16)
        assert all(g[k].dtype == np.float64 for k in dc.TENSORS)
        if name != "const":
            assert all(0 < float(g["fp32_dev_" + k]) < 2e-4 for k in dc.TENSORS)


# ------------------------------------------------------------------------------------------ the switch
def _args():
    return NS(multires=10, multires_views=4, i_embed=0, backbone2d_fpn_dim=32, model_3d_hidden_dim=32,
              render=NS(N_samples=16, N_importance=0, N_rand=1024, chunk=2048, lindisp=False, white_bkgd=False, use_render_uncertainty=True, render_feature=True),
              use_scene_coord_memorization=False, matcher_hidden_dim=192, use_depth_supervision=False, matching=NS(fine_num_3d_keypoints=1024))


def test_the_switch_is_off_by_default():
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    assert DepthFusionNet.hip_encode is False and DepthFusionNet().hip_encode is False
    assert "hip_encode" not in DepthFusionNet().__dict__   # a class attribute until an instance sets it
    assert ConditionalNeRF(_args()).multiview_aggregator.depth_fusion.hip_encode is False
    net = ConditionalNeRF(_args(), hip_frame_cnn=True)
    assert net.multiview_aggregator.depth_fusion.hip_encode is True and DepthFusionNet.hip_encode is False
    assert set(net.state_dict()) == set(ConditionalNeRF(_args()).state_dict())   # the cache adds nothing to the checkpoint


def test_with_the_switch_set_cpu_tensors_and_grad_wanting_calls_stay_eager(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library path was taken")
    monkeypatch.setattr(_cnn_lib, "dfnet_forward", no_library)
    monkeypatch.setattr(_cnn_lib, "pack_weights", no_library)
    x, _ = dc.build("wide")
    x = torch.from_numpy(x)
    eager, hip = build_module("wide"), build_module("wide")
    hip.hip_encode = True
    with torch.no_grad():
        want = eager.encode(x)
        assert torch.equal(hip.encode(x), want)                      # a CPU tensor
        assert torch.equal(hip.encode(x.double().float()), want)
        hip64 = build_module("wide").double()
        hip64.hip_encode = True
        assert hip64.encode(x.double()).dtype == torch.float64      # another dtype
        odd = torch.from_numpy(dc.make_input(1, 32, 32, 3))[:, :, :, :]
        assert hip.encode(odd).shape == (1, 32, 8, 8)
    got = hip.encode(x)                                              # gradients wanted: the parameters require them
    assert got.requires_grad and torch.equal(got.detach(), want)
    got.sum().backward()
    assert hip.conv_out.weight.grad is not None and hip.pack_count == 0
    assert hip._use_hip(x) is False
