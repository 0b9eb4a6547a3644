"""CPU-side tests of appearance adaptation (nerf_loc_amd/appearance.py, _app_lib.py, include/nerfloc_app.h) against tests/golden/app_*.npz — the outputs of the
reference's AppearanceEmbedding and AppearanceAdaptLayer on the recipes of tests/appearance_cases.py (tools/gen_appearance_golden.py) — and of the third library's
boundary.  Errors are max |a - b| / max |b| with b the reference."""
import ctypes as ct
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _app_lib, _head_lib, _lib
from nerf_loc_amd.appearance import AppearanceAdaptLayer, AppearanceEmbedding
from tests import appearance_cases as ac
from tests import appearance_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4        # the project's parity bar
RESTATED = 1e-12  # fp64 restatement against the reference's fp64
HEADER = os.path.join(ROOT, "include", "nerfloc_app.h")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def stats_case(name):
    return ac.make_stats_case(name)


@functools.lru_cache(maxsize=None)
def adapt_case(name):
    return ac.make_adapt_case(name)


@functools.lru_cache(maxsize=None)
def golden(name):
    return ac.load_golden(name)


def build_layer(name, device="cpu"):
    c = adapt_case(name)
    m = AppearanceAdaptLayer(ac.Args(), c["case"].C, is_rgb=c["case"].is_rgb)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    return m.to(device)


def weights_of(c):
    return [c["state"][k] for k in ac.PARAM_NAMES]


# ------------------------------------------------------------------------------------------ the third library's boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nla_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_app_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_app_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 8 and "nla_channel_stats" in declared and "nla_film_backward" in declared
    assert sorted(n for n, _, _ in _app_lib.SYMBOLS) == declared
    assert _exported(_app_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no nl_* / nlh_* symbol
    lib = _app_lib.load()
    hdr = open(HEADER).read()
    assert lib.nla_abi_version() == _app_lib.ABI_VERSION == int(re.search(r"#define\s+NLA_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    for name, val in (("NLA_LAYOUT_NCHW", _app_lib.LAYOUT_NCHW), ("NLA_LAYOUT_NHWC", _app_lib.LAYOUT_NHWC), ("NLA_ADAPT_HIDDEN", _app_lib.HIDDEN)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1)) == val
    assert int(re.search(r"#define\s+NLA_FILM_CLIP01\s+(\d+)u", hdr).group(1)) == _app_lib.FILM_CLIP01


def test_the_other_two_libraries_export_no_app_symbol():
    assert not [n for n in _exported(_lib.LIB_PATH) + _exported(_head_lib.LIB_PATH) if n.startswith("nla_")]


@pytest.fixture(scope="module")
def host():
    """(lib, p): p a 256-byte aligned HOST address that no call below may read — every call here is refused (or has nothing to do) before a launch."""
    buf = (ct.c_char * 8192)()
    return _app_lib.load(), (ct.addressof(buf) + 255) // 256 * 256, buf


def test_channel_stats_refuses_bad_arguments_without_a_device(host):
    lib, p, _ = host
    N, H = _app_lib.LAYOUT_NCHW, _app_lib.LAYOUT_NHWC
    need = lib.nla_channel_stats_workspace_bytes(3, 64, 240, N)
    assert need == 3 * 64 * 1 * 8 and lib.nla_channel_stats_workspace_bytes(1, 64, 76800, N) == 64 * 19 * 8
    assert lib.nla_channel_stats_workspace_bytes(1, 64, 76800, H) == 64 * 300 * 8
    for bad in ((3, 64, 1, N), (3, 0, 240, N), (3, 1025, 240, N), (3, 64, 240, 2), (-1, 64, 240, N), (0, 64, 240, N), (3, 64, (1 << 30) + 1, N)):
        assert lib.nla_channel_stats_workspace_bytes(*bad) == 0, bad
    call = lambda x, B, C, HW, lay, out, ws, wsb: lib.nla_channel_stats(x, B, C, HW, lay, out, ws, wsb, None)
    E = _lib.NL_ERR_BAD_ARG
    assert call(p, 3, 64, 1, N, p, p, need) == E            # HW = 1
    assert call(p, 3, 0, 240, N, p, p, need) == E           # C = 0
    assert call(p, -1, 64, 240, N, p, p, need) == E
    assert call(p, 3, 64, 240, 2, p, p, need) == E          # unknown layout
    assert call(p, 3, 1025, 240, H, p, p, need) == _lib.NL_ERR_UNSUPPORTED
    assert call(p, 3, 64, (1 << 30) + 1, N, p, p, need) == _lib.NL_ERR_UNSUPPORTED
    assert call(None, 3, 64, 240, N, p, p, need) == E and call(p, 3, 64, 240, N, None, p, need) == E
    assert call(p + 2, 3, 64, 240, N, p, p, need) == E and call(p, 3, 64, 240, N, p + 1, p, need) == E   # wrong alignment
    W = _lib.NL_ERR_WORKSPACE
    assert call(p, 3, 64, 240, N, p, None, need) == W and call(p, 3, 64, 240, N, p, p, need - 1) == W and call(p, 3, 64, 240, N, p, p + 16, need) == W
    assert call(None, 0, 64, 240, N, None, None, 0) == _lib.NL_OK   # B == 0: nothing to do


def test_adapt_code_refuses_bad_arguments_without_a_device(host):
    lib, p, _ = host
    w = (ct.c_void_p * 6)(*([p] * 6))
    call = lambda emb, tgt, wts, V, E, C, code: lib.nla_adapt_code(emb, tgt, wts, V, E, C, code, None)
    B = _lib.NL_ERR_BAD_ARG
    assert call(p, p, w, 3, 6, 64, p) == B and call(p, p, w, 3, 0, 64, p) == B      # E = 6, E = 0
    assert call(p, p, w, 3, 128, 0, p) == B and call(p, p, w, -1, 128, 64, p) == B   # C = 0
    assert call(p, p, w, 3, 516, 64, p) == _lib.NL_ERR_UNSUPPORTED and call(p, p, w, 3, 128, 1025, p) == _lib.NL_ERR_UNSUPPORTED
    assert call(None, p, w, 3, 128, 64, p) == B and call(p, None, w, 3, 128, 64, p) == B and call(p, p, None, 3, 128, 64, p) == B and call(p, p, w, 3, 128, 64, None) == B
    assert call(p + 2, p, w, 3, 128, 64, p) == B
    hole = (ct.c_void_p * 6)(p, p, p, None, p, p)
    odd = (ct.c_void_p * 6)(p, p, p + 2, p, p, p)
    assert call(p, p, hole, 3, 128, 64, p) == B and call(p, p, odd, 3, 128, 64, p) == B
    assert call(None, None, None, 0, 128, 64, None) == _lib.NL_OK   # V == 0


def test_film_refuses_bad_arguments_without_a_device(host):
    lib, p, _ = host
    film = lambda x, code, V, HW, C, flags, y: lib.nla_film(x, code, V, HW, C, flags, y, None)
    B, U = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED
    assert film(p, p, 3, 35, 0, 0, p) == B and film(p, p, 3, 0, 64, 0, p) == B and film(p, p, -1, 35, 64, 0, p) == B
    assert film(p, p, 3, 35, 64, 2, p) == B and film(p, p, 3, 35, 64, 0x80000001, p) == B   # unknown flag bits
    assert film(p, p, 3, 35, 1025, 0, p) == U and film(p, p, 4, 1 << 30, 256, 0, p) == U    # C = 1025; V HW C = 2^40
    assert film(None, p, 3, 35, 64, 0, p) == B and film(p, None, 3, 35, 64, 0, p) == B and film(p, p, 3, 35, 64, 0, None) == B
    assert film(p + 2, p, 3, 35, 64, 0, p) == B and film(p, p, 3, 35, 64, 0, p + 1) == B
    assert film(None, None, 0, 35, 64, 1, None) == _lib.NL_OK   # V == 0
    assert lib.nla_film_backward_block_pixels(192) == 160 and lib.nla_film_backward_block_pixels(3) == 85 * 32 and lib.nla_film_backward_block_pixels(1024) == 32
    assert lib.nla_film_backward_block_pixels(0) == 0 and lib.nla_film_backward_block_pixels(1025) == 0
    need = lib.nla_film_backward_workspace_bytes(3, 5000, 192)
    assert need == 3 * 32 * 384 * 4 and lib.nla_film_backward_workspace_bytes(3, 35, 3) == 256
    for bad in ((3, 0, 64), (3, 35, 0), (3, 35, 1025), (-1, 35, 64), (0, 35, 64), (4, 1 << 30, 256)):
        assert lib.nla_film_backward_workspace_bytes(*bad) == 0, bad
    bwd = lambda x, code, gy, V, HW, C, flags, gx, gc, ws, wsb: lib.nla_film_backward(x, code, gy, V, HW, C, flags, gx, gc, ws, wsb, None)
    assert bwd(p, p, p, 3, 5000, 0, 0, p, p, p, need) == B and bwd(p, p, p, 3, 0, 192, 0, p, p, p, need) == B
    assert bwd(p, p, p, 3, 5000, 192, 4, p, p, p, need) == B and bwd(p, p, p, 3, 5000, 1025, 0, p, p, p, need) == U
    assert bwd(None, p, p, 3, 5000, 192, 0, p, p, p, need) == B and bwd(p, None, p, 3, 5000, 192, 0, p, p, p, need) == B and bwd(p, p, None, 3, 5000, 192, 0, p, p, p, need) == B
    assert bwd(p, p, p + 2, 3, 5000, 192, 0, p, p, p, need) == B and bwd(p, p, p, 3, 5000, 192, 0, p + 2, p, p, need) == B and bwd(p, p, p, 3, 5000, 192, 0, p, p + 1, p, need) == B
    W = _lib.NL_ERR_WORKSPACE
    assert bwd(p, p, p, 3, 5000, 192, 0, p, p, None, need) == W and bwd(p, p, p, 3, 5000, 192, 0, p, p, p, need - 1) == W and bwd(p, p, p, 3, 5000, 192, 0, p, p, p + 128, need) == W
    assert bwd(p, p, p, 3, 5000, 192, 1, None, None, None, 0) == _lib.NL_OK   # neither cotangent wanted: nothing to do
    assert bwd(None, None, None, 0, 5000, 192, 0, None, None, None, 0) == _lib.NL_OK   # V == 0


# ------------------------------------------------------------------------------------------ the restatement reproduces the goldens
@pytest.mark.parametrize("name", list(ac.STATS_CASES))
def test_restated_statistics_equal_the_reference(name):
    c, g = stats_case(name), golden(f"stats_{name}")
    got = ar.channel_stats(c["conv1"])
    n = c["case"].c
    em, es = rel(got[:, :n], g["out"][:, :n]), rel(got[:, n:], g["out"][:, n:])
    print(f"stats {name}: restatement vs reference fp64: mean {em:.2e}, std {es:.2e} (reference fp32 vs fp64 {float(g['dev_mean']):.2e}, {float(g['dev_std']):.2e})")
    assert em <= RESTATED and es <= RESTATED


def test_sum_of_squares_in_fp32_fails_the_offset_case_and_two_passes_do_not():
    """Why the contract names its formulation: on `offset` the textbook variance in fp32 is wrong by more than the value; two passes are at rounding level."""
    c, g = stats_case("offset"), golden("stats_offset")
    x = c["conv1"].reshape(c["case"].B, c["case"].c, -1)
    n = np.float32(x.shape[2])
    want = g["out"][:, c["case"].c:]
    m = x.sum(axis=2, dtype=np.float32) / n
    naive = np.sqrt(np.maximum((x * x).sum(axis=2, dtype=np.float32) / n - m * m, 0) * (n / (n - 1)))
    d = x - m[:, :, None]
    two = np.sqrt((d * d).sum(axis=2, dtype=np.float32) / (n - 1))
    print(f"offset: E[x^2] - E[x]^2 in fp32 {rel(naive, want):.2e}, two passes in fp32 {rel(two, want):.2e}")
    assert rel(naive, want) > 100 * BAR and rel(two, want) <= 1e-5


@pytest.mark.parametrize("name", list(ac.ADAPT_CASES))
def test_restated_adapt_layer_equals_the_reference(name):
    c, g = adapt_case(name), golden(f"adapt_{name}")
    case = c["case"]
    code, z1, z2 = ar.adapt_code(c["embedding"], c["target_embedding"], weights_of(c), pre=True)
    assert min(np.abs(z1).min(), np.abs(z2).min()) > ac.SAFE_MARGIN
    assert rel(code, g["code"]) <= RESTATED
    y = ar.film(c["x"], g["code"], case.is_rgb)
    assert rel(y, g["y"]) <= RESTATED
    g_x, g_code = ar.film_backward(c["x"], g["code"], c["g_y"], case.is_rgb)
    assert rel(g_x, g["grad_x"]) <= RESTATED and rel(g_code, g["grad_code"]) <= RESTATED
    rest = ar.adapt_backward(c["embedding"], c["target_embedding"], weights_of(c), g_code)
    for k in ac.GRAD_NAMES[1:]:
        assert rel(rest[k], g["grad_" + k]) <= RESTATED, k
    if case.is_rgb:
        m = ar.clip_mask(c["x"], g["code"])
        assert 0.02 < 1.0 - m.mean() < 0.98 and abs((1.0 - m.mean()) - float(g["clipped"])) < 1e-12
        assert np.array_equal(g["grad_x"] != 0, m)   # a is never 0 and g_y is never 0 in these recipes: the stored gradient shows the reference's mask


# ------------------------------------------------------------------------------------------ the modules on CPU tensors
@pytest.mark.parametrize("name", list(ac.STATS_CASES))
def test_embedding_on_cpu_gives_the_reference(name):
    c, g = stats_case(name), golden(f"stats_{name}")
    n = c["case"].c
    mod = AppearanceEmbedding(ac.Args(2 * n))
    assert not list(mod.parameters()) and not list(mod.buffers()) and not mod.state_dict()
    conv1 = torch.from_numpy(c["conv1"])
    if c["case"].channels_last:
        conv1 = conv1.contiguous(memory_format=torch.channels_last)
    out = mod(None, {"conv1": conv1})
    assert tuple(out.shape) == (c["case"].B, 2 * n) and out.dtype == torch.float32
    assert rel(out[:, :n].numpy(), g["out"][:, :n]) <= BAR and rel(out[:, n:].numpy(), g["out"][:, n:]) <= BAR
    with pytest.raises(AssertionError):
        AppearanceEmbedding(ac.Args(2 * n + 2))(None, {"conv1": conv1})


@pytest.mark.parametrize("hip_training", [True, False])
@pytest.mark.parametrize("name", list(ac.ADAPT_CASES))
def test_adapt_layer_on_cpu_gives_the_reference_outputs_and_nine_gradients(name, hip_training):
    c, g = adapt_case(name), golden(f"adapt_{name}")
    m = build_layer(name)   # strict=True inside
    m.hip_training = hip_training
    sd = m.state_dict()
    assert list(sd.keys()) == g["state_dict_names"].tolist() == list(ac.PARAM_NAMES)
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == g["state_dict_shapes"].tolist()
    ins = {k: torch.from_numpy(c[k]).requires_grad_(True) for k in ("x", "embedding", "target_embedding")}
    y = m.train()(ins["x"], ins["embedding"], ins["target_embedding"])
    assert y.shape == ins["x"].shape and rel(y.detach().numpy(), g["y"]) <= BAR
    (torch.from_numpy(c["g_y"]) * y).sum().backward()
    grads = {k: v.grad.numpy() for k, v in ins.items()}
    grads.update({k: p.grad.numpy() for k, p in m.named_parameters()})
    for k in ac.GRAD_NAMES:
        err = rel(grads[k], g["grad_" + k])
        print(f"{name} grad {k}: {err:.2e}")
        assert err <= BAR, k
    with torch.no_grad():
        y_eval = m.eval()(ins["x"], ins["embedding"], ins["target_embedding"][0])   # an (E,) target broadcasts as (1, E)
    assert torch.equal(y_eval, y.detach())
    if c["case"].is_rgb:
        assert np.array_equal((y_eval.numpy() > 0) & (y_eval.numpy() < 1), ar.clip_mask(c["x"], g["code"]))


def test_hip_training_is_a_class_attribute_and_eval_on_cpu_needs_no_library_call(monkeypatch):
    assert AppearanceAdaptLayer.hip_training is True
    for fn in ("channel_stats", "adapt_code", "film", "film_backward"):
        monkeypatch.setattr(_app_lib, fn, lambda *a, **k: pytest.fail("the library was called for CPU tensors"))
    c = adapt_case("c64")
    with torch.no_grad():
        build_layer("c64").eval()(torch.from_numpy(c["x"]), torch.from_numpy(c["embedding"]), torch.from_numpy(c["target_embedding"]))
    AppearanceEmbedding(ac.Args())(None, {"conv1": torch.from_numpy(stats_case("plain")["conv1"])})
