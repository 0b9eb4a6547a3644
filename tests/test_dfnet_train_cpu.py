"""The eighth library's boundary and the training switch of DepthFusionNet, without a GPU: header against binding against symbol table, the weight names, the
size queries and their stated arithmetic, refusals decided on the host, the numpy stage restatement against torch's fp64 autograd, and the in-repo eager module's
fp64 gradients against the reference's fixtures — which makes that module the truth of the GPU tests at every shape without a fixture."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_loc_amd import _cabi, _cnn_lib, _cnn_train_lib, _lib
from nerf_loc_amd.depth_fusion import DepthFusionNet
from tests import dfnet_cases as dc
from tests import dfnet_train_cases as tc
from tests import dfnet_train_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerfloc_cnn_train.h")
EAGER_AGAINST_REFERENCE = 1e-10


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlct_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_train_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_cnn_train_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 11 and "nlct_dfnet_forward_train" in declared and "nlct_dfnet_backward" in declared
    assert sorted(n for n, _, _ in _cnn_train_lib.SYMBOLS) == declared
    assert _exported(_cnn_train_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no nlc_ symbol
    lib = _cnn_train_lib.load()
    hdr = open(HEADER).read()
    assert lib.nlct_abi_version() == _cnn_train_lib.ABI_VERSION == int(re.search(r"#define\s+NLCT_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    sig = {n: (r, a) for n, r, a in _cnn_train_lib.SYMBOLS}
    V, I, Z = ct.c_void_p, ct.c_int, ct.c_size_t
    assert sig["nlct_dfnet_forward_train"] == (I, [V, V, I, I, I, V, V, Z, V])
    assert sig["nlct_dfnet_backward"] == (I, [V, V, I, I, I, V, V, ct.POINTER(V), V, Z, V])
    assert sig["nlct_dfnet_pack_weights"] == (I, [ct.POINTER(V), I, V, Z, V])
    assert sig["nlct_conv_backward"] == (I, [V, I, V, I, V, V, I, I, I, I, I, I, V, V, V, V, Z, V])
    assert sig["nlct_up2_backward"] == (I, [V, I, I, I, V, V])
    # no hand-written argtypes in the binding
    src = open(os.path.join(ROOT, "nerf_loc_amd", "_cnn_train_lib.py")).read()
    assert "argtypes" not in src and "restype" not in src
    assert _cabi.struct_fields("nerfloc_cnn_train.h") == {}


def test_the_inference_library_keeps_its_seven_symbols():
    assert len(_exported(_cnn_lib.LIB_PATH)) == 7 and not [n for n in _exported(_cnn_lib.LIB_PATH) if n.startswith("nlct_")]
    assert _cnn_lib.load().nlc_abi_version() == 1


def test_weight_names_are_the_state_dict_keys_and_the_image_extends_the_inference_image():
    assert _cnn_lib.weight_names() == list(DepthFusionNet().state_dict().keys())
    lib = _cnn_train_lib.load()
    nb, base = lib.nlct_dfnet_packed_bytes(), _cnn_lib.load().nlc_dfnet_packed_bytes()
    sd = DepthFusionNet().state_dict()
    trans = sum((v.numel() + 63) // 64 * 64 for k, v in sd.items() if v.dim() == 4 and v.shape[1] >= 32 and k.startswith("fuse_net.") and "out_conv" not in k)
    assert nb % 256 == 0 and nb == (base + 4 * trans + 255) // 256 * 256


def _state_floats(V, H, W):
    """The header's list."""
    up = lambda n: (n + 63) // 64 * 64
    n0, n1 = (H // 2 - 1) * (W // 2 - 1), (H // 4) * (W // 4)
    tot = 2 * up(V * 32 * n0) + up(V * 32 * 4)
    for L in range(3):
        C, n = 32 << L, n1 >> (2 * L)
        tot += 9 * up(V * C * n) + 5 * up(V * C * 4)
    tot += up(V * 128 * (n1 // 4)) + 4 * up(V * 64 * (n1 // 4)) + up(V * 64 * n1) + 4 * up(V * 32 * n1)
    return tot + 2 * up(V * 64 * 4) + 2 * up(V * 32 * 4)


def test_size_queries_answer_zero_outside_the_limits_and_follow_the_stated_arithmetic():
    lib = _cnn_train_lib.load()
    for V, H, W in ((1, 32, 32), (2, 32, 48), (3, 48, 80), (5, 256, 336), (64, 1024, 1024)):
        sb, wb = lib.nlct_dfnet_state_bytes(V, H, W), lib.nlct_dfnet_backward_workspace_bytes(V, H, W)
        assert sb == (4 * _state_floats(V, H, W) + 255) // 256 * 256 and wb > 0 and wb % 256 == 0
    for V, H, W in ((0, 32, 32), (65, 32, 32), (1, 16, 32), (1, 32, 16), (1, 40, 64), (1, 36, 48), (-1, 32, 32), (64, 1024, 1040)):
        assert lib.nlct_dfnet_state_bytes(V, H, W) == 0 and lib.nlct_dfnet_backward_workspace_bytes(V, H, W) == 0
    q = lib.nlct_conv_backward_workspace_bytes
    assert q(2, 32, 32, 64, 5, 3, 3, 1) > 0 and q(1, 12, 0, 32, 32, 48, 8, 2) > 0 and q(1, 32, 0, 32, 2, 2, 3, 2) > 0
    for bad in ((0, 32, 0, 32, 8, 8, 3, 1), (1, 32, 0, 32, 8, 8, 5, 1), (1, 32, 0, 32, 8, 8, 3, 3), (1, 32, 0, 32, 1, 8, 3, 1), (1, 600, 0, 32, 8, 8, 3, 1),
                (1, 12, 0, 32, 2, 8, 8, 2), (65, 32, 0, 32, 8, 8, 3, 1)):
        assert q(*bad) == 0, bad


def test_refusals_are_decided_without_a_device():
    lib = _cnn_train_lib.load()
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 255) // 256 * 256   # a HOST address no call below may read: every call here is refused before a launch
    U, B, Wk = _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_WORKSPACE
    sb, wb = lib.nlct_dfnet_state_bytes(1, 32, 32), lib.nlct_dfnet_backward_workspace_bytes(1, 32, 32)
    fwd = lambda packed, x, V, H, W, out, st, n: lib.nlct_dfnet_forward_train(packed, x, V, H, W, out, st, n, None)
    assert fwd(p, p, 1, 40, 64, p, p, 1 << 40) == U and fwd(p, p, 0, 32, 32, p, p, 1 << 40) == U
    assert fwd(None, p, 1, 32, 32, p, p, sb) == B and fwd(p, None, 1, 32, 32, p, p, sb) == B and fwd(p, p, 1, 32, 32, None, p, sb) == B
    assert fwd(p, p + 4, 1, 32, 32, p, p, sb) == B
    assert fwd(p, p, 1, 32, 32, p, None, sb) == Wk and fwd(p, p, 1, 32, 32, p, p, sb - 1) == Wk and fwd(p, p, 1, 32, 32, p, p + 16, sb) == Wk
    grads = (ct.c_void_p * 72)(*([p] * 72))
    bwd = lambda packed, x, V, H, W, st, g, gr, ws, n: lib.nlct_dfnet_backward(packed, x, V, H, W, st, g, gr, ws, n, None)
    assert bwd(p, p, 1, 40, 64, p, p, grads, p, 1 << 40) == U
    assert bwd(p, p, 1, 32, 32, None, p, grads, p, wb) == B and bwd(p, p, 1, 32, 32, p, None, grads, p, wb) == B and bwd(p, p, 1, 32, 32, p, p, None, p, wb) == B
    assert bwd(p, p, 1, 32, 32, p, p, grads, None, wb) == Wk and bwd(p, p, 1, 32, 32, p, p, grads, p, wb - 1) == Wk and bwd(p, p, 1, 32, 32, p, p, grads, p + 16, wb) == Wk
    grads[7] = p + 2
    assert bwd(p, p, 1, 32, 32, p, p, grads, p, wb) == B
    ptrs = (ct.c_void_p * 72)(*([p] * 72))
    nb = lib.nlct_dfnet_packed_bytes()
    assert lib.nlct_dfnet_pack_weights(ptrs, 71, p, nb, None) == B and lib.nlct_dfnet_pack_weights(None, 72, p, nb, None) == B
    assert lib.nlct_dfnet_pack_weights(ptrs, 72, p, nb - 1, None) == Wk and lib.nlct_dfnet_pack_weights(ptrs, 72, p + 16, nb, None) == Wk
    ptrs[5] = None
    assert lib.nlct_dfnet_pack_weights(ptrs, 72, p, nb, None) == B
    # the stages
    cw = lib.nlct_conv_backward_workspace_bytes(1, 32, 0, 32, 8, 8, 3, 1)
    conv = lambda x0, C0, x1, C1, w, gy, V, co, h, wd, ks, s, g0, g1, gw, ws, n: lib.nlct_conv_backward(x0, C0, x1, C1, w, gy, V, co, h, wd, ks, s, g0, g1, gw, ws, n, None)
    assert conv(p, 32, None, 0, p, p, 1, 32, 8, 8, 5, 1, p, None, p, p, cw) == U
    assert conv(p, 12, None, 0, p, p, 1, 32, 32, 32, 8, 2, p, None, p, p, 1 << 30) == U    # conv1 has no data gradient
    assert conv(p, 32, None, 0, p, p, 1, 48, 8, 8, 3, 1, p, None, p, p, 1 << 30) == U      # nor a convolution with cout % 32 != 0
    assert conv(p, 32, None, 0, p, None, 1, 32, 8, 8, 3, 1, p, None, p, p, cw) == B and conv(p, 32, None, 0, p, p, 1, 32, 8, 8, 3, 1, p, p, p, p, cw) == B
    assert conv(p, 32, None, 0, p, p, 1, 32, 8, 8, 3, 1, p, None, p, p, cw - 1) == Wk and conv(p, 32, None, 0, p, p, 1, 32, 8, 8, 3, 1, p, None, p, None, cw) == Wk
    inb = lambda x, nrm, y, act, g, V, C, n, gx, gg, gb, ws, nby: lib.nlct_instnorm_backward(x, nrm, y, act, g, V, C, n, gx, gg, gb, ws, nby, None)
    assert inb(p, p, p, 1, p, 0, 4, 4, p, p, p, p, 256) == U and inb(p, p, p, 3, p, 1, 4, 4, p, p, p, p, 256) == B
    assert inb(p, p, None, 1, p, 1, 4, 4, p, p, p, p, 256) == B and inb(p, p, None, 0, p, 1, 4, 4, p, p, p, p, 31) == Wk
    assert lib.nlct_up2_backward(p, 1, 1, 4, p, None) == U and lib.nlct_up2_backward(None, 1, 2, 4, p, None) == B


def test_the_switch_is_off_by_default_and_cpu_calls_stay_eager(monkeypatch):
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    from tests.test_dfnet_cpu import _args
    assert DepthFusionNet.hip_training is False and "hip_training" not in DepthFusionNet().__dict__
    assert ConditionalNeRF(_args()).multiview_aggregator.depth_fusion.hip_training is False
    net = ConditionalNeRF(_args(), hip_frame_cnn_training=True)
    assert net.multiview_aggregator.depth_fusion.hip_training is True and net.multiview_aggregator.depth_fusion.hip_encode is False
    assert DepthFusionNet.hip_training is False and set(net.state_dict()) == set(ConditionalNeRF(_args()).state_dict())

    def no_library(*a, **k):
        raise AssertionError("the library path was taken")
    monkeypatch.setattr(_cnn_train_lib, "dfnet_forward_train", no_library)
    monkeypatch.setattr(_cnn_train_lib, "pack_weights", no_library)
    m = DepthFusionNet()
    m.hip_training = True
    x = torch.from_numpy(dc.make_input(1, 32, 32, 3))
    m.encode(x).sum().backward()    # a CPU tensor: eager
    assert m.conv_out.weight.grad is not None and m.pack_count == 0 and m._use_hip_training(x) is False


# ------------------------------------------------------------------------------------------ the stage restatement against torch's fp64 autograd
@pytest.mark.parametrize("ks,stride,hin,win", [(3, 1, 2, 2), (3, 2, 3, 5), (1, 2, 5, 3), (8, 2, 16, 24), (3, 2, 23, 39)])
def test_restated_conv_backward_equals_autograd(ks, stride, hin, win):
    rng = np.random.default_rng(ks * 100 + hin)
    x, w = rng.standard_normal((2, 6, hin, win)), rng.standard_normal((4, 6, ks, ks))
    xt, wt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w).requires_grad_()
    pad = tr.PAD[ks]
    y = F.conv2d(F.pad(xt, (pad,) * 4, mode="reflect") if pad else xt, wt, stride=stride)
    g = rng.standard_normal(tuple(y.shape))
    (y * torch.from_numpy(g)).sum().backward()
    g_x, g_w = tr.conv_backward(x, w, g, stride)
    assert tc.rel(g_x, xt.grad.numpy()) <= 1e-12 and tc.rel(g_w, wt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("act", [0, 1, 2])
def test_restated_instnorm_and_up2_backward_equal_autograd(act):
    rng = np.random.default_rng(act)
    x, gamma, beta = rng.standard_normal((2, 3, 15)), rng.uniform(0.5, 2, 3), rng.standard_normal(3)
    xt, gt, bt = (torch.from_numpy(a).requires_grad_() for a in (x, gamma, beta))
    y = F.instance_norm(xt, weight=gt, bias=bt, eps=1e-5)
    y = y if act == 0 else F.relu(y) if act == 1 else F.elu(y)
    g = rng.standard_normal(x.shape)
    (y * torch.from_numpy(g)).sum().backward()
    nrm = tr.make_norm(x, gamma, beta).astype(np.float64)
    mean = x.mean(axis=2)
    rstd = 1 / np.sqrt(((x - mean[..., None]) ** 2).mean(axis=2) + 1e-5)
    nrm = np.stack([mean, gamma[None] * rstd, np.broadcast_to(beta[None], mean.shape), rstd], axis=2)   # fp64: the formulas, not the rounding, are under test
    g_x, g_gamma, g_beta = tr.instnorm_backward(x, nrm, tr.act_of(x, nrm, act), act, g)
    assert tc.rel(g_x, xt.grad.numpy()) <= 1e-11 and tc.rel(g_gamma, gt.grad.numpy()) <= 1e-11 and tc.rel(g_beta, bt.grad.numpy()) <= 1e-11
    u = torch.from_numpy(rng.standard_normal((1, 2, 3, 5))).requires_grad_()
    gu = rng.standard_normal((1, 2, 6, 10))
    (F.interpolate(u, scale_factor=2, mode="bilinear", align_corners=True) * torch.from_numpy(gu)).sum().backward()
    assert tc.rel(tr.up2_backward(gu[0]), u.grad.numpy()[0]) <= 1e-12


# ------------------------------------------------------------------------------------------ the in-repo eager module against the reference's gradients
def eager_grads(x, w, cot, dtype):
    m = DepthFusionNet().to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in w.items()}, strict=True)
    (m.encode(torch.from_numpy(x).to(dtype)) * torch.from_numpy(cot).to(dtype)).sum().backward()
    return {k: p.grad.double().numpy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", tc.RECIPES)
def test_eager_fp64_autograd_meets_the_reference_fixture(name):
    x, w = dc.build(name)
    V, H, W = dc.CASES[name][:3]
    g, got = tc.fixture(name), eager_grads(x, w, tc.cotangent(V, H, W), torch.float64)
    assert len(got) == 72 and sum(v.size for v in got.values()) == 908216
    worst = 0.0
    for k, v in got.items():
        if k in tc.ZERO_BIASES:
            assert float(g["fp32_dev_" + k]) == 0.0 and not g["grad_" + k].any()
            assert np.abs(v).max() < 1e-10   # autograd's rounding noise around an exact zero
            continue
        e = tc.rel(v, tc.fixture_fp64(g, k))
        worst = max(worst, e)
        assert e <= EAGER_AGAINST_REFERENCE, (name, k, e)
        assert tc.rel(g["grad_" + k], v) <= 2.0 ** -24    # the fp32 tensor the GPU tests read is that gradient rounded
    print(name, "eager fp64 against the reference's fp64: worst %.3g" % worst)


def test_fixture_records_the_bars_of_the_issue():
    for name, worst in (("wide", 4.7e-5), ("odd5", 2.0e-5)):
        g = tc.fixture(name)
        devs = {k[9:]: float(v) for k, v in g.items() if k.startswith("fp32_dev_")}
        assert len(devs) == 72 and max(devs, key=devs.get) == "fuse_net.layer3.0.bn1.weight"
        assert abs(max(devs.values()) / worst - 1) < 0.05
