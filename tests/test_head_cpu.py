"""CPU-side tests of the localisation head as one object (nerf_loc_amd/matcher.py, position_encoding.py, _head_lib.py) against tests/golden/head_*.npz — the
outputs of the reference's Matcher, PositionEmbeddingSine and get_embedder on the recipes of tests/head_cases.py (tools/gen_head_golden.py) — and of the second
library's boundary (include/nerfloc_head.h).  Errors are max |a - b| / max |b| with b the reference."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _head_lib, _lib
from nerf_loc_amd.matcher import Matcher
from nerf_loc_amd.position_encoding import PositionEmbeddingSine, get_embedder
from tests import head_cases as hc
from tests import head_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4   # the project's parity bar


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def case(name):
    return hc.make_case(name)


@functools.lru_cache(maxsize=None)
def golden(name):
    return hc.load_golden(name)


def build_matcher(name, **kw):
    c = case(name)
    C = c["case"].C
    m = Matcher(hc.Args, C, C, C, **kw)
    state = {k: torch.from_numpy(v) for k, v in c["state"].items()}
    if not kw.get("fine_matching", True):
        state = {k: v for k, v in state.items() if k.startswith("coarse_")}
    m.load_state_dict(state, strict=True)
    return m


def zero_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
        if hasattr(mod, "dim_feedforward") and hasattr(mod, "dropout") and isinstance(mod.dropout, float):
            mod.dropout = 0.0   # SelfCrossTransformer's own record of the probability (read by its library training step)
    return m


def tensors(data, device="cpu", grads=()):
    out = {}
    for k, v in data.items():
        if isinstance(v, np.ndarray):
            t = torch.from_numpy(v).to(device)
            if k in grads:
                t.requires_grad_(True)
            out[k] = t
        else:
            out[k] = v
    return out


# ------------------------------------------------------------------------------------------ the restatement reproduces the goldens
@pytest.mark.parametrize("C", hc.POS_CHANNELS)
def test_restated_position_tables_equal_the_reference(C):
    g = golden(f"pos_c{C}")
    for H, W in hc.POS_SHAPES:
        want = g[f"pos_{H}x{W}"]
        got = hr.pos_sine_grid(H, W, C)
        assert got.shape == want.shape == (H, W, C) and got.dtype == np.float32
        err = rel(got, want)
        print(f"pos {H}x{W} C {C}: restatement vs reference {err:.2e} (reference fp32 vs fp64 {float(g[f'dev_{H}x{W}']):.2e})")
        assert err <= 1e-6
        if f"pos64_{H}x{W}" in g:
            assert rel(hr.pos_sine_grid(H, W, C, np.float64), g[f"pos64_{H}x{W}"]) <= 1e-12


def test_restated_embedder_equals_the_reference():
    g = golden("embed")
    assert int(g["out_dim"]) == 2 * 3 * hc.EMBED_L
    for n in (1, 65):
        x = hc.embed_points_input(n)
        if n == 65:
            assert np.array_equal(x.reshape(-1)[:7], np.array(hc.EMBED_SPECIAL, dtype=np.float32))
        got = hr.embed_points(x, hc.EMBED_L)
        err32, err64 = rel(got, g[f"embed_{n}"]), rel(got, g[f"embed64_{n}"])
        print(f"embed N {n}: restatement vs reference fp32 {err32:.2e}, fp64 {err64:.2e}")
        assert got.shape == g[f"embed_{n}"].shape and err32 <= 1e-6 and err64 <= 1e-6


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_restated_selection_equals_the_reference_exactly(name):
    c, g = case(name), golden(name)
    d = c["data"]
    N, Mc = c["case"].N, len(d["kps2d"])
    match_j = np.full(N, -1, dtype=np.int32)
    match_j[g["i_ids"]] = g["j_ids"]
    M = len(g["i_ids"])
    for cap in (N, M, M - 3):
        r = hr.select_matches(match_j, cap, Mc, d["kps3d"], d["kps2d"], d["desc_3d_fine"], d["pos_emd_3d"])
        k = min(cap, M)
        assert r["info"].tolist() == [k, M, int(M > cap), 0]
        assert np.array_equal(r["i_ids"][:k], g["i_ids"][:k]) and np.array_equal(r["j_ids"][:k], g["j_ids"][:k]) and not r["b_ids"].any()
        assert np.array_equal(r["mkps3d"][:k], g["mkps3d"][:k]) and np.array_equal(r["mkps2d_c"][:k], g["mkps2d_c"][:k])
        assert np.array_equal(r["out_a"][:k], d["desc_3d_fine"][g["i_ids"][:k]]) and np.array_equal(r["out_b"][:k], d["pos_emd_3d"][g["i_ids"][:k]])
        for key in ("i_ids", "j_ids", "mkps3d", "mkps2d_c", "out_a", "out_b"):
            assert not r[key][k:].any(), key
    # an entry outside [0, Mc) is unmatched
    bad = match_j.copy()
    bad[g["i_ids"][0]] = Mc
    bad[g["i_ids"][1]] = -5
    r = hr.select_matches(bad, N, Mc, d["kps3d"], d["kps2d"])
    assert r["info"].tolist() == [M - 2, M - 2, 0, 0] and np.array_equal(r["i_ids"][:M - 2], g["i_ids"][2:]) and r["out_a"] is None


# ------------------------------------------------------------------------------------------ the second library's boundary
def _declared():
    src = open(os.path.join(ROOT, "include", "nerfloc_head.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nlh_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_head_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_head_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 7 and "nlh_select_matches" in declared and "nlh_pnp_ransac_counted" in declared
    assert sorted(n for n, _, _ in _head_lib.SYMBOLS) == declared
    assert _exported(_head_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no nl_* symbol
    lib = _head_lib.load()
    hdr = open(os.path.join(ROOT, "include", "nerfloc_head.h")).read()
    assert lib.nlh_abi_version() == _head_lib.ABI_VERSION == int(re.search(r"#define\s+NLH_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1


def test_render_library_exports_no_head_symbol():
    names = _exported(_lib.LIB_PATH)
    assert len(names) == 104 and all(n.startswith("nl_") for n in names) and names == sorted(n for n, _, _ in _lib.SYMBOLS)


def test_head_library_refuses_bad_arguments_without_a_device():
    """The checks that come before any launch (host pointers that are never read)."""
    import ctypes as ct
    lib = _head_lib.load()
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 255) // 256 * 256
    assert lib.nlh_select_workspace_bytes(0) == 0 and lib.nlh_select_workspace_bytes((1 << 20) + 1) == 0 and lib.nlh_select_workspace_bytes(1100) == 256
    sel = lambda N, cap, Mc, C, ra, ws, wsb: lib.nlh_select_matches(p, N, cap, Mc, C, p, p, ra, None, p, p, p, p, p, p, None, p, ws, wsb, None)
    assert sel(0, 4, 4, 64, p, p, 256) == _lib.NL_ERR_BAD_ARG and sel(4, 0, 4, 64, p, p, 256) == _lib.NL_ERR_BAD_ARG
    assert sel(4, 4, 4, 66, p, p, 256) == _lib.NL_ERR_BAD_ARG and sel(4, 4, 4, 516, p, p, 256) == _lib.NL_ERR_UNSUPPORTED
    assert sel(4, 4, 4, 64, p + 4, p, 256) == _lib.NL_ERR_BAD_ARG
    assert sel(4, 4, 4, 64, p, None, 256) == _lib.NL_ERR_WORKSPACE and sel(4, 4, 4, 64, p, p + 8, 256) == _lib.NL_ERR_WORKSPACE
    assert sel(4, 4, 4, 64, p, p, 0) == _lib.NL_ERR_WORKSPACE
    assert lib.nlh_pos_sine_grid(3, 5, 6, p, None) == _lib.NL_ERR_BAD_ARG and lib.nlh_pos_sine_grid(0, 5, 8, p, None) == _lib.NL_ERR_BAD_ARG
    assert lib.nlh_embed_points(p, 4, 3, 33, p, None) == _lib.NL_ERR_UNSUPPORTED and lib.nlh_embed_points(p, 4, 0, 4, p, None) == _lib.NL_ERR_BAD_ARG
    assert lib.nlh_embed_points(None, 0, 3, 32, None, None) == _lib.NL_OK
    off = (ct.c_int32 * 2)(0, 10)
    K = (ct.c_double * 4)(500.0, 500.0, 320.0, 240.0)
    thr = (ct.c_double * 1)(8.0)
    need = lib.nlh_pnp_workspace_bytes(10, 1, 64)
    assert need == _lib.load().nl_pnp_workspace_bytes(10, 1, 64) > 0 and lib.nlh_pnp_workspace_bytes(10, 1, 100) == 0
    call = lambda cnt, H, mi, ws, wsb: lib.nlh_pnp_ransac_counted(p, p, off, cnt, K, thr, 1, H, 0, mi, p, p, p, None, ws, wsb, None)
    assert call(None, 64, 4, p, need) == _lib.NL_ERR_BAD_ARG and call(p, 64, 3, p, need) == _lib.NL_ERR_BAD_ARG
    assert call(p, 100, 4, p, need) == _lib.NL_ERR_UNSUPPORTED and call(p, 64, 4, p, need - 1) == _lib.NL_ERR_WORKSPACE


# ------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_state_dict_has_the_reference_names_and_loads_strictly(name):
    g = golden(name)
    m = build_matcher(name)   # strict=True inside
    sd = m.state_dict()
    assert len(sd) == 118 and list(sd.keys()) == g["state_dict_names"].tolist()
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == g["state_dict_shapes"].tolist()
    assert len(list(m.pos_emd_2d_fn.parameters())) == 0 and len(list(m.pos_emd_2d_fn.buffers())) == 0
    coarse = build_matcher(name, fine_matching=False)
    assert list(coarse.state_dict().keys()) == [k for k in g["state_dict_names"].tolist() if k.startswith("coarse_")]


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_training_mode_on_cpu_gives_the_reference_losses_and_gradients(name):
    c = case(name)
    with np.load(os.path.join(hc.golden_dir(), f"head_{name}_train.npz")) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(hc.golden_dir(), f"head_{name}_train_map.npz")) as z:
        g["grad_feat_fine"] = z["grad_feat_fine"]
    m = zero_dropout(build_matcher(name)).train()
    data = tensors(c["data"], grads=hc.INPUT_GRADS)
    out = m(data)
    assert sorted(set(out) - set(c["data"])) == g["train_keys"].tolist()
    assert np.array_equal(out["expec_f_gt"].detach().numpy(), g["expec_f_gt"]) and np.array_equal(out["i_ids"].numpy(), c["data"]["pairs_gt"][0])
    (out["coarse_loss"] + out["fine_loss"]).backward()
    for k in ("coarse_loss", "fine_loss", "fine_err"):
        err = abs(out[k].item() - float(g[k + "_64"])) / abs(float(g[k + "_64"]))
        print(f"{name} {k}: {out[k].item():.6f} vs {float(g[k + '_64']):.6f}: {err:.2e}")
        assert err <= BAR, k
    for k in hc.INPUT_GRADS:
        err = rel(data[k].grad.numpy(), g["grad_" + k])
        print(f"{name} grad {k}: {err:.2e}")
        assert err <= BAR, k


def test_eval_mode_on_cpu_tensors_raises():
    m = build_matcher("head64").eval()
    data = tensors(case("head64")["data"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(data)
    for fn in (m.forward_padded, lambda d: m.localize(d, (500.0, 500.0, 32.0, 24.0), 8.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(data)
    with pytest.raises(RuntimeError, match="eval mode with fine matching only"):
        m.train().forward_padded(data)
    with pytest.raises(RuntimeError, match="eval mode with fine matching only"):
        build_matcher("head64", fine_matching=False).eval().forward_padded(data)


@pytest.mark.parametrize("C", hc.POS_CHANNELS)
def test_position_classes_give_the_goldens_on_cpu(C):
    g = golden(f"pos_c{C}")
    mod = PositionEmbeddingSine(C // 2, normalize=True, sine_type="lin_sine")
    for H, W in hc.POS_SHAPES:
        out = mod(torch.zeros(2, H, W))
        assert tuple(out.shape) == (2, H, W, C) and torch.equal(out[0], out[1])
        assert rel(out[0].numpy(), g[f"pos_{H}x{W}"]) <= 1e-6
    ge = golden("embed")
    fn, dim = get_embedder(hc.EMBED_L, 0, include_input=False)
    assert dim == int(ge["out_dim"])
    for n in (1, 65):
        assert rel(fn(torch.from_numpy(hc.embed_points_input(n))).numpy(), ge[f"embed_{n}"]) <= 1e-6
    fn_in, dim_in = get_embedder(4, 0, include_input=True)
    x = torch.from_numpy(hc.embed_points_input(5))
    assert dim_in == 27 and torch.equal(fn_in(x)[:, :3], x) and tuple(fn_in(x).shape) == (5, 27)
