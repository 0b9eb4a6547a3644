"""The ninth library's boundary and the counted matcher's argument checks, without a GPU: header against export map against symbol table against binding, the
neighbouring libraries' pins, the numpy restatement of the counted selection against tests/match_ref.py's rule on the truncated matrix, refusals decided on the
host, and the Python entry points' refusals (a host count, CPU tensors, training mode)."""
import ctypes as ct
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _cabi, _counted_lib, _head_lib, _lib, cascade
from nerf_loc_amd.matcher import Matcher
from nerf_loc_amd.matching import S2DMatching
from nerf_loc_amd.transformer import SelfCrossTransformer
from tests import counted_ref as cr
from tests import head_cases as hc
from tests import match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerfloc_counted.h")
DECLARED = ["nlk_abi_version", "nlk_s2d_select_counted", "nlk_s2d_select_workspace_bytes", "nlk_sct_forward_counted", "nlk_sct_layer_counted",
            "nlk_sct_workspace_bytes"]


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlk_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_header_export_map_symbol_table_and_binding_agree():
    assert os.path.exists(_counted_lib.LIB_PATH), "run __graft_entry__.build() first"
    assert _declared() == DECLARED
    assert sorted(n for n, _, _ in _counted_lib.SYMBOLS) == DECLARED
    assert _exported(_counted_lib.LIB_PATH) == DECLARED   # nothing else: no kernel stubs, no nl_ symbol
    emap = open(os.path.join(ROOT, "nerf_loc_amd", "csrc", "exports_counted.map")).read()
    assert re.findall(r"global:\s*([^;]+);", emap) == ["nlk_*"] and re.findall(r"local:\s*([^;]+);", emap) == ["*"]
    lib = _counted_lib.load()
    assert lib.nlk_abi_version() == _counted_lib.ABI_VERSION == int(re.search(r"#define\s+NLK_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 1
    sig = {n: (r, a) for n, r, a in _counted_lib.SYMBOLS}
    V, I, L, Z, F = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_size_t, ct.c_float
    assert sig["nlk_sct_workspace_bytes"] == (Z, [L, L, L, I, I])
    assert sig["nlk_sct_forward_counted"] == (I, [V, I, I, I, I, V, V, L, V, V, V, L, L, V, V, V, Z, V])
    assert sig["nlk_sct_layer_counted"] == (I, [V, I, I, I, I, I, V, V, L, V, V, L, V, L, V, V, Z, V])
    assert sig["nlk_s2d_select_counted"] == (I, [V, L, L, V, F, V, V, V, Z, V])
    src = open(os.path.join(ROOT, "nerf_loc_amd", "_counted_lib.py")).read()
    assert "argtypes" not in src and "restype" not in src   # no hand-written signature in the binding
    assert _cabi.struct_fields("nerfloc_counted.h") == {}


def test_the_render_and_head_libraries_keep_their_symbols_and_abi():
    render, head = _exported(_lib.LIB_PATH), _exported(_head_lib.LIB_PATH)
    assert len(render) == 104 and len(head) == 7 and not [n for n in render + head if n.startswith("nlk_")]
    assert _lib.load().nl_abi_version() == 13 and _head_lib.load().nlh_abi_version() == 1


def test_workspace_queries_follow_the_render_library_and_the_stated_arithmetic():
    lib, base = _counted_lib.load(), _lib.load()
    for args in ((1, 544, 40, 64, 64), (2, 130, 48, 64, 64), (1, 1024, 4800, 192, 512), (0, 5, 5, 64, 64), (1, 0, 5, 64, 64), (1, 1 << 25, 5, 64, 64)):
        assert lib.nlk_sct_workspace_bytes(*args) == base.nl_sct_workspace_bytes(*args), args
    up = lambda b: (b + 255) // 256 * 256
    for N, M in ((1, 1), (65, 48), (130, 200), (1100, 70), (1024, 4800)):
        assert lib.nlk_s2d_select_workspace_bytes(N, M) == up(4 * N) + up(4 * M)
    for N, M in ((0, 5), (5, 0), (-1, 5), ((1 << 30) + 1, 1), (1 << 30, 1 << 30)):
        assert lib.nlk_s2d_select_workspace_bytes(N, M) == 0


def test_refusals_are_decided_without_a_device():
    lib = _counted_lib.load()
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 255) // 256 * 256   # a HOST address no call below may read: every call here is refused before a launch
    U, B, Wk = _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_WORKSPACE
    wb = lib.nlk_sct_workspace_bytes(1, 8, 8, 64, 64)
    fwd = lambda packed, C, nh, F, prec, v0, N0, n0, v1, N1, Bn, o0, o1, ws, n: lib.nlk_sct_forward_counted(packed, C, nh, F, prec, v0, p, N0, n0, v1, p, N1, Bn, o0, o1,
                                                                                                         ws, n, None)
    assert fwd(p, 64, 8, 64, 1, p, 0, p, p, 8, 1, p, p + 256, p, wb) == B          # an empty sequence
    assert fwd(p, 96, 8, 64, 1, p, 8, p, p, 8, 1, p, p + 256, p, wb) == U          # d_model outside the set
    assert fwd(p, 64, 4, 64, 1, p, 8, p, p, 8, 1, p, p + 256, p, wb) == U          # nhead
    assert fwd(p, 64, 8, 64, 3, p, 8, p, p, 8, 1, p, p + 256, p, wb) == U          # f16mx
    assert fwd(p, 64, 8, 64, 7, p, 8, p, p, 8, 1, p, p + 256, p, wb) == B          # no precision at all
    assert fwd(None, 64, 8, 64, 1, p, 8, p, p, 8, 1, p, p + 256, p, wb) == B
    assert fwd(p, 64, 8, 64, 1, None, 8, p, p, 8, 1, p, p + 256, p, wb) == B and fwd(p, 64, 8, 64, 1, p + 4, 8, p, p, 8, 1, p, p + 256, p, wb) == B
    assert fwd(p, 64, 8, 64, 1, p, 8, p + 2, p, 8, 1, p, p + 256, p, wb) == B      # a misaligned count
    assert fwd(p, 64, 8, 64, 1, p, 8, p, p, 8, 1, p, p, p, wb) == B                # out0 == out1
    assert fwd(p, 64, 8, 64, 1, p, 8, p, p, 8, 1, p, p + 256, None, wb) == Wk and fwd(p, 64, 8, 64, 1, p, 8, p, p, 8, 1, p, p + 256, p, wb - 1) == Wk
    assert fwd(p, 64, 8, 64, 1, p, 8, p, p, 8, 1, p, p + 256, p + 16, wb) == Wk
    assert fwd(p, 64, 8, 64, 1, p, 8, p, p, 8, 0, p, p + 256, None, 0) == _lib.NL_OK   # an empty batch: nothing is launched
    lay = lambda layer, x, Nq, mem, Nk, nk, ws, n: lib.nlk_sct_layer_counted(p, 64, 8, 64, layer, 1, x, p, Nq, mem, None if mem is None else p, Nk, nk, 1, p, ws, n, None)
    assert lay(4, p, 8, None, 8, p, p, wb) == B and lay(-1, p, 8, None, 8, p, p, wb) == B
    assert lay(0, p, 8, None, 9, p, p, wb) == B and lay(0, p, 8, p + 256, 8, p, p, wb) == B     # a self layer with another memory side
    assert lay(2, p, 8, None, 8, p, p, wb) == B and lay(2, p, 8, p, 8, p + 1, p, wb) == B
    assert lay(2, p, 8, p, 8, p, p, wb - 1) == Wk
    sb = lib.nlk_s2d_select_workspace_bytes(8, 8)
    sel = lambda s, N, M, n, mj, ms, ws, nb: lib.nlk_s2d_select_counted(s, N, M, n, 0.2, mj, ms, ws, nb, None)
    assert sel(p, 0, 8, p, p, p, p, sb) == B and sel(p, 8, (1 << 30) + 1, p, p, p, p, 1 << 40) == U
    assert sel(None, 8, 8, p, p, p, p, sb) == B and sel(p, 8, 8, p, None, p, p, sb) == B and sel(p, 8, 8, p, p, None, p, sb) == B
    assert sel(p, 8, 8, p + 2, p, p, p, sb) == B and sel(p + 1, 8, 8, p, p, p, p, sb) == B
    assert sel(p, 8, 8, p, p, p, None, sb) == Wk and sel(p, 8, 8, p, p, p, p, sb - 1) == Wk and sel(p, 8, 8, p, p, p, p + 16, sb) == Wk


# ------------------------------------------------------------------------------------------ the restatement of the counted selection
def _padded(s, n, seed):
    """s cut to n rows, then rows that would win every column maximum if they counted."""
    rng = np.random.default_rng(seed)
    out = s.copy()
    out[n:] = np.minimum(out[rng.integers(0, max(n, 1), size=len(s) - n)] * np.float32(8), np.float32(1.0)) if n else np.float32(1.0)
    return out


@pytest.mark.parametrize("N,M", [(1, 1), (7, 5), (65, 48), (130, 200)])
@pytest.mark.parametrize("kind", ["random", "tied"])
def test_restated_counted_selection_equals_the_rule_on_the_truncated_matrix(N, M, kind):
    rng = np.random.default_rng(N * 1000 + M)
    s = cr.tied_scores(N, M, N + M) if kind == "tied" else (1 / (1 + np.exp(-3 * rng.standard_normal((N, M))))).astype(np.float32)
    thr = 0.2
    if kind == "tied" and N >= 3 and M >= 4:   # the planted ties are what they claim to be
        full = mr.select(s, thr)
        assert full[0] == 1 and full[1] == 2 and full[2] == 2 and (s[0] == s[0].max()).sum() == 2
    for n in sorted({0, 1, N // 2, N, N + 3, -2}):
        k = cr.clamp_count(n, N)
        sp = _padded(s, k, n + 11)
        mj, ms = cr.select_counted(sp, n, thr)
        want = mr.select(s[:k], thr) if k else np.zeros(0, dtype=np.int64)
        assert mj.dtype == np.int32 and ms.dtype == np.float32
        assert np.array_equal(mj[:k], want) and (mj[k:] == -1).all() and not ms[k:].any()
        assert np.array_equal(ms[:k], np.where(want >= 0, s[:k].max(axis=1) if k else 0, 0).astype(np.float32))
        if 0 < k < N and (want >= 0).any():   # the mask matters: the plain rule on the padded matrix loses matches to the padded rows
            assert not np.array_equal(mr.select(sp, thr)[:k], want)


# ------------------------------------------------------------------------------------------ the Python entry points' refusals
def test_signatures_default_to_the_uncounted_path():
    for fn, name in ((SelfCrossTransformer.transform, "n0"), (S2DMatching.match, "n"), (Matcher.forward_padded, "num_points"), (Matcher.localize, "num_points")):
        assert inspect.signature(fn).parameters[name].default is None
    p = inspect.signature(cascade.localize_cascade).parameters
    assert list(p)[:7] == ["matcher", "matcher_fine", "data", "K", "H", "W", "thr"] and p["hypotheses"].default == 1024 and p["seed"].default == 0
    assert p["min_inliers"].default == 4


def test_a_host_count_and_a_cpu_count_are_refused():
    for bad in (3, np.int32(3), 3.0):
        with pytest.raises(TypeError, match="DEVICE tensor"):
            _counted_lib.device_count(bad, "t")
    for bad in (torch.tensor(3, dtype=torch.int32), torch.tensor(3), torch.tensor([3, 4], dtype=torch.int32)):
        with pytest.raises(ValueError, match="int32"):
            _counted_lib.device_count(bad, "t")
    m = Matcher(hc.Args, 64, 64, 64).eval()
    data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in hc.make_case("head64")["data"].items()}
    with pytest.raises(TypeError, match="DEVICE tensor"):
        m.forward_padded(data, num_points=3)
    with pytest.raises(TypeError, match="DEVICE tensor"):
        m.localize(data, (100.0, 100.0, 40.0, 30.0), 24.0, num_points=3)
    with pytest.raises(ValueError, match="int32"):
        m.localize(data, (100.0, 100.0, 40.0, 30.0), 24.0, num_points=torch.tensor(3, dtype=torch.int32))


def test_cpu_tensors_and_training_mode_are_refused():
    m, mf = Matcher(hc.Args, 64, 64, 64).eval(), Matcher(hc.Args, 64, 64, 64).eval()
    data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in hc.make_case("head64")["data"].items()}
    K = (100.0, 100.0, 40.0, 30.0)
    with pytest.raises(ValueError, match="HIP tensors"):
        cascade.localize_cascade(m, mf, data, K, 60, 80, 24.0)
    mf.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        cascade.localize_cascade(m, mf, data, K, 60, 80, 24.0)
    with pytest.raises(RuntimeError, match="eval mode"):
        mf.forward_padded(data)
    t = SelfCrossTransformer(d_model=64, nhead=8, dim_feedforward=64).eval()
    x = torch.zeros(1, 4, 64)
    for n0 in (None, torch.tensor(2, dtype=torch.int32)):   # CPU tensors: no CPU fallback, with or without a count
        with pytest.raises(RuntimeError, match="only on a HIP device"):
            t.transform(x, x, x, x, n0=n0)
