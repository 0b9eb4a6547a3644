"""CPU-side tests of the keypoint geometry (nerf_loc_amd/keypoints.py, _geom_lib.py, include/nerfloc_geom.h): the fourth library's boundary, and the fp64
restatement (tests/geom_ref.py) and the eager CPU path against tests/golden/geom_*.npz — the outputs of the reference's select_3d_keypoints / build_3d_2d_pairs on
the recipes of tests/geom_cases.py (tools/gen_geom_golden.py).  Decisions are exact on every point; proj is max |a - b| / max |b| with b the reference's fp64."""
import ctypes as ct
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _app_lib, _cabi, _geom_lib, _head_lib, _lib, keypoints as kp
from tests import geom_cases as gc
from tests import geom_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4   # the project's parity bar
HEADER = os.path.join(ROOT, "include", "nerfloc_geom.h")


@functools.lru_cache(maxsize=None)
def case(name):
    return gc.make_case(name)


@functools.lru_cache(maxsize=None)
def want(name):
    return gc.expected(case(name), gc.load_golden(name))


# ------------------------------------------------------------------------------------------ the fourth library's boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlg_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_geom_header_parses_through_the_binding_layer():
    P, I, L, Z, F, D, U = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_size_t, ct.c_float, ct.c_double, ct.c_uint
    protos = _cabi.prototypes("nerfloc_geom.h", "nlg_")
    assert protos == _geom_lib.SYMBOLS and len(protos) == 7
    assert sorted(n for n, _, _ in protos) == _declared()
    by_name = {n: (r, a) for n, r, a in protos}
    assert by_name["nlg_select_visible"] == (I, [P, L, P, I, P, I, I, U, L, P, P, P, P, Z, P])   # typed out by hand
    assert by_name["nlg_build_pairs"] == (I, [P, L, P, P, I, I, I, D, P, U, L, P, P, P, P, P, P, P, P, Z, P])
    assert by_name["nlg_conf_target"] == (I, [P, L, L, I, L, L, P, P]) and by_name["nlg_cell_grid"] == (I, [I, I, F, P, P])
    assert by_name["nlg_build_pairs_workspace_bytes"] == (Z, [L]) and not _cabi.struct_fields("nerfloc_geom.h")
    d = _cabi.defines("nerfloc_geom.h")
    assert (d["NLG_POSE_F32"], d["NLG_POSE_F64"], d["NLG_DEPTH_MAP"], d["NLG_DEPTH_POINTS"]) == (0, 1, 0, 2) and d["NLG_MAX_VIEWS"] == 64
    assert d["NLG_MAX_POINTS"] == 1 << 20 and d["NLG_MIN_POSITIVES"] == gr.MIN_POSITIVES == kp.MIN_POSITIVES == 4


def test_geom_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_geom_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 7 and "nlg_select_visible" in declared and "nlg_conf_target" in declared
    assert _exported(_geom_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no symbol of another library
    lib = _geom_lib.load()
    hdr = open(HEADER).read()
    assert lib.nlg_abi_version() == _geom_lib.ABI_VERSION == int(re.search(r"#define\s+NLG_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1


def test_the_other_three_libraries_export_no_geom_symbol_and_keep_their_counts():
    for mod, count in ((_lib, 104), (_head_lib, 7), (_app_lib, 8)):
        names = _exported(mod.LIB_PATH)
        assert len(names) == count and not [n for n in names if n.startswith("nlg_")]


@pytest.fixture(scope="module")
def host():
    """(lib, p): p a 256-byte aligned HOST address that no call below may read — every call here is refused (or has nothing to do) before a launch."""
    buf = (ct.c_char * 8192)()
    return _geom_lib.load(), (ct.addressof(buf) + 255) // 256 * 256, buf


def test_select_visible_refuses_bad_arguments_without_a_device(host):
    lib, p, _ = host
    B, U, Wk = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    assert lib.nlg_select_visible_workspace_bytes(1) == 256 and lib.nlg_select_visible_workspace_bytes(256 * 64 + 1) == 512
    assert lib.nlg_select_visible_workspace_bytes(1 << 20) == 4096 * 4
    assert lib.nlg_select_visible_workspace_bytes(0) == 0 and lib.nlg_select_visible_workspace_bytes((1 << 20) + 1) == 0
    need = lib.nlg_select_visible_workspace_bytes(1000)
    call = lambda pts=p, N=1000, poses=p, V=3, K=p, H=48, W=64, flags=0, cap=1000, mask=p, idx=p, info=p, ws=p, wsb=need: \
        lib.nlg_select_visible(pts, N, poses, V, K, H, W, flags, cap, mask, idx, info, ws, wsb, None)
    assert call(N=0) == B and call(V=0) == B and call(H=0) == B and call(W=-1) == B and call(cap=0) == B and call(flags=2) == B and call(flags=4) == B
    assert call(V=65) == U and call(N=(1 << 20) + 1) == U and call(H=(1 << 15) + 1) == U and call(cap=(1 << 24) + 1) == U
    for null in ("pts", "poses", "K", "mask", "idx", "info"):
        assert call(**{null: None}) == B, null
    assert call(pts=p + 2) == B and call(idx=p + 4) == B and call(poses=p + 4, flags=1) == B
    assert call(ws=None) == Wk and call(wsb=need - 1) == Wk and call(ws=p + 16) == Wk


def test_build_pairs_refuses_bad_arguments_without_a_device(host):
    lib, p, _ = host
    B, U, Wk = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    assert lib.nlg_build_pairs_workspace_bytes(1000) == 256 and lib.nlg_build_pairs_workspace_bytes(1 << 20) == 2 * 4096 * 4
    assert lib.nlg_build_pairs_workspace_bytes(0) == 0 and lib.nlg_build_pairs_workspace_bytes((1 << 20) + 1) == 0
    need = lib.nlg_build_pairs_workspace_bytes(1000)
    names = ("proj", "z", "valid", "pos", "gt_j", "pairs", "info")

    def call(pts=p, N=1000, pose=p, K=p, H=48, W=64, stride=8, thr=0.05, depth=p, flags=0, cap=1000, ws=p, wsb=need, **outs):
        o = [outs.get(n, p) for n in names]
        return lib.nlg_build_pairs(pts, N, pose, K, H, W, stride, thr, depth, flags, cap, *o, ws, wsb, None)
    assert call(N=0) == B and call(stride=0) == B and call(cap=0) == B and call(flags=4) == B and call(H=0) == B
    assert call(stride=7) == B and call(H=50) == B and call(W=65, stride=5) == B   # stride does not divide H / W
    assert call(N=(1 << 20) + 1) == U and call(W=1 << 16, stride=1) == U
    for null in ("pts", "pose", "K", "depth") + names:
        assert call(**{null: None}) == B, null
    assert call(pairs=p + 4) == B and call(pose=p + 4, flags=1) == B and call(depth=p + 1, flags=2) == B
    assert call(ws=None) == Wk and call(wsb=need - 1) == Wk and call(ws=p + 128) == Wk


def test_conf_target_and_cell_grid_refuse_bad_arguments_without_a_device(host):
    lib, p, _ = host
    B, U = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED
    tgt = lambda gt=p, N=64, M=160, dtype=0, b=0, e=64, out=p: lib.nlg_conf_target(gt, N, M, dtype, b, e, out, None)
    assert tgt(N=0) == B and tgt(M=0) == B and tgt(dtype=2) == B and tgt(b=-1) == B and tgt(b=3, e=2) == B and tgt(e=65) == B
    assert tgt(N=(1 << 24) + 1) == U and tgt(M=(1 << 24) + 1) == U
    assert tgt(gt=None) == B and tgt(out=None) == B and tgt(out=p + 2) == B and tgt(out=p + 4, dtype=1) == B
    assert tgt(gt=None, out=None, b=5, e=5) == _lib.NL_OK   # an empty range: nothing to do
    grid = lambda Hc=6, Wc=8, out=p: lib.nlg_cell_grid(Hc, Wc, 1.0, out, None)
    assert grid(Hc=0) == B and grid(Wc=0) == B and grid(out=None) == B and grid(out=p + 4) == B and grid(Hc=(1 << 15) + 1) == U


# ------------------------------------------------------------------------------------------ the goldens
def check(name, mask, idx, pairs_out):
    """Holds one implementation's outputs (numpy) to the golden of `name`: decisions exactly, proj at the bar."""
    c, w = case(name), want(name)
    assert np.array_equal(mask, w["mask"]) and np.array_equal(idx, w["vis_idx"])
    n = w["pairs"].shape[1]
    assert int(pairs_out["num"]) == n and np.array_equal(pairs_out["pairs"][:, :n], w["pairs"]) and not pairs_out["pairs"][:, n:].any()
    assert np.array_equal(pairs_out["valid"], w["valid"]) and np.array_equal(pairs_out["gt_j"], w["gt_j"])
    assert int(pairs_out["used_fallback"]) == w["used_fallback"]
    pos = pairs_out["pos"]
    assert not (pos & ~w["valid"]).any() and (np.array_equal(np.nonzero(pos)[0], w["pairs"][0]) or w["used_fallback"])
    assert gc.proj_error(pairs_out["proj"], w["proj64"]) <= BAR and gc.proj_error(pairs_out["proj"], w["proj64"], w["valid"]) <= BAR
    if c["case"].kind == "edge":   # exact coordinates: the same bits, NaN and inf included
        assert np.array_equal(pairs_out["proj"], w["proj64"].astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    c = case(name)
    k = c["case"]
    mask, idx, info = gr.select_visible(c["pts"], c["poses"], c["K"], k.H, k.W)
    assert info[0] == info[1] == mask.sum() and not info[2] and not idx[info[0]:].any()
    out = gr.build_pairs(c["pts"], c["query"], c["K"], k.H, k.W, k.stride, k.thr, c["depth"], c["depth_points"])
    out["num"], out["used_fallback"] = out["info"][0], out["info"][3]
    check(name, mask, idx[:info[0]], out)
    g = gc.load_golden(name)
    assert np.array_equal(gr.cell_grid(k.H // k.stride, k.W // k.stride), g["grid"].astype(np.float32))
    assert gc.proj_error(g["proj"], g["proj64"], want(name)["valid"]) <= BAR   # the reference's own fp32 run, for scale


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_eager_cpu_path_reproduces_the_reference(name, monkeypatch):
    for fn in ("select_visible", "build_pairs", "conf_target", "cell_grid"):
        monkeypatch.setattr(_geom_lib, fn, lambda *a, **k: pytest.fail("the library was called for CPU tensors"))
    c = case(name)
    k = c["case"]
    t = torch.from_numpy
    idx = kp.select_3d_keypoints(t(c["pts"]), [t(p) for p in c["poses"]], t(c["K"]), k.H, k.W)
    assert idx.dtype == torch.int64
    pidx, mask, num, overflow = kp.select_3d_keypoints_padded(t(c["pts"]), t(c["poses"]).double(), t(c["K"]), k.H, k.W)
    assert int(num) == len(idx) and not int(overflow) and torch.equal(pidx[:len(idx)], idx) and not pidx[len(idx):].any()
    depth = {"depth_points": t(c["depth"])} if c["depth_points"] else {"depth_map": t(c["depth"])}
    out = kp.build_3d_2d_pairs_padded(t(c["pts"]), k.H, k.W, t(c["K"]), t(c["query"]), k.thr, k.stride, **depth)
    check(name, mask.numpy(), idx.numpy(), {n: v.numpy() for n, v in out.items()})
    pts, grid, proj, pairs = kp.build_3d_2d_pairs(t(c["pts"]), k.H, k.W, t(c["K"]), t(c["query"]), k.thr, k.stride, **depth)
    g = gc.load_golden(name)
    assert pts.data_ptr() == t(c["pts"]).data_ptr() and grid.dtype == torch.int64 and np.array_equal(grid.numpy(), g["grid"])
    assert np.array_equal(pairs.numpy(), want(name)["pairs"]) and np.array_equal(proj.numpy(), out["proj"].numpy(), equal_nan=True)
    # the target of these pairs, both dtypes, against the reference's formulation: zeros + index-put of the pairs
    M = (k.H // k.stride) * (k.W // k.stride)
    dense = np.zeros((k.N, M), dtype=np.int64)
    dense[want(name)["pairs"][0], want(name)["pairs"][1]] = 1
    assert np.array_equal(kp.conf_matrix_target(out["gt_j"], M, torch.int64).numpy(), dense)
    f = kp.conf_matrix_target(out["gt_j"], M)
    assert f.dtype == torch.float32 and np.array_equal(f.numpy(), dense.astype(np.float32)) and np.array_equal(gr.conf_target(out["gt_j"].numpy(), M), f.numpy())


@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_no_point_of_a_fixture_is_left_out(name):
    g = gc.load_golden(name)
    assert float(g["excluded_share"]) == 0.0 and gc.excluded_share(case(name)) == 0.0
    assert np.array_equal(g["band"], [gc.BAND_PX, gc.BAND_Z, gc.BAND_DEPTH]) and int(g["N"]) == case(name)["case"].N <= 2048
    if case(name)["case"].kind != "edge":
        assert gc.BAND_PX >= 8 * float(g["dev_uv_px"]) and gc.BAND_Z >= 8 * float(g["dev_z"])
    assert os.path.getsize(os.path.join(gc.golden_dir(), f"geom_{name}.npz")) < 200 * 1024


def test_eager_path_pads_and_flags_overflow():
    c = case("small")
    k = c["case"]
    t = torch.from_numpy
    n = len(want("small")["vis_idx"])
    idx, _, num, overflow = kp.select_3d_keypoints_padded(t(c["pts"]), t(c["poses"]), t(c["K"]), k.H, k.W, capacity=5)
    assert n > 5 and int(num) == 5 and int(overflow) == 1 and np.array_equal(idx.numpy(), want("small")["vis_idx"][:5])
    ref = gr.select_visible(c["pts"], c["poses"], c["K"], k.H, k.W, cap=5)
    assert np.array_equal(ref[1], idx.numpy()) and list(ref[2]) == [5, n, 1, 0]
    with pytest.raises(ValueError, match="exactly one"):
        kp.build_3d_2d_pairs(t(c["pts"]), k.H, k.W, t(c["K"]), t(c["query"]), k.thr, k.stride)
    with pytest.raises(ValueError, match="stride"):
        kp.build_3d_2d_pairs(t(c["pts"]), k.H, k.W, t(c["K"]), t(c["query"]), k.thr, 7, depth_map=t(c["depth"]))
