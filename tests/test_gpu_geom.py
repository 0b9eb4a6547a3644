"""GPU tests of the keypoint geometry: libnerfloc_geom.so's entry points and the drop-ins of nerf_loc_amd/keypoints.py against tests/golden/geom_*.npz (the
reference's decisions, exactly, on every point) and against the fp64 restatement tests/geom_ref.py at the shapes where the scan and the stores can go wrong."""
import functools

import numpy as np
import pytest
import torch

from nerf_loc_amd import _geom_lib, _lib, keypoints as kp
from nerf_loc_amd.matching import S2DMatching
from tests import geom_cases as gc
from tests import geom_ref as gr

pytestmark = pytest.mark.gpu
BAR = 1e-4   # the project's parity bar
H, W, STRIDE, THR = 48, 64, 8, 0.05   # the image of the sweeps
SECOND_LEVEL = _geom_lib.CHUNK * 1024 + 1   # the scan's 1024 threads own one chunk of 256 points each up to here; one point more and each owns two


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return gc.make_case(name)


@functools.lru_cache(maxsize=None)
def sweep(N, V):
    """Inputs of one sweep shape and what the restatement makes of them, computed once."""
    pts, poses, query, K = gc.sweep_inputs(N, V, 100 + N % 97 + V)
    depth = gc.sweep_depth(pts, query, K, H, W, THR, 7, True)
    return {"pts": pts, "poses": poses, "query": query, "K": K, "depth": depth, "vis": gr.select_visible(pts, poses, K, H, W),
            "pairs": gr.build_pairs(pts, query, K, H, W, STRIDE, THR, depth, True)}


def same_pairs(out, ref, proj_bits=True):
    """The library's build_pairs dict (numpy) against the restatement's: every integer and mask exactly; proj / z to the bit (the same fp64 operations, one rounding)."""
    for k in ("valid", "pos", "gt_j", "pairs", "info"):
        assert np.array_equal(out[k], ref[k]), k
    if proj_bits:
        assert np.array_equal(out["proj"], ref["proj"], equal_nan=True) and np.array_equal(out["z"], ref["z"], equal_nan=True)


# ------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("pose_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", gc.GOLDEN_CASES)
def test_library_takes_the_references_decisions_on_every_point(name, pose_dtype):
    c, k = case(name), case(name)["case"]
    w = gc.expected(c, gc.load_golden(name))
    mask, idx, info = _geom_lib.select_visible(dev(c["pts"]), dev(c["poses"], pose_dtype), dev(c["K"]), k.H, k.W)
    n = len(w["vis_idx"])
    assert info.tolist() == [n, n, 0, 0] and np.array_equal(mask.cpu().numpy(), w["mask"])
    assert np.array_equal(idx[:n].cpu().numpy(), w["vis_idx"]) and not idx[n:].any()
    out = host(_geom_lib.build_pairs(dev(c["pts"]), dev(c["query"], pose_dtype), dev(c["K"]), k.H, k.W, k.stride, k.thr, dev(c["depth"]), c["depth_points"]))
    p = w["pairs"].shape[1]
    assert out["info"].tolist() == [p, p, 0, w["used_fallback"]]
    assert np.array_equal(out["pairs"][:, :p], w["pairs"]) and not out["pairs"][:, p:].any()
    assert np.array_equal(out["valid"], w["valid"]) and np.array_equal(out["gt_j"], w["gt_j"])
    assert not (out["pos"] & ~w["valid"]).any() and (w["used_fallback"] or np.array_equal(np.nonzero(out["pos"])[0], w["pairs"][0]))
    assert gc.proj_error(out["proj"], w["proj64"]) <= BAR and gc.proj_error(out["proj"], w["proj64"], w["valid"]) <= BAR
    ref = gr.build_pairs(c["pts"], c["query"], c["K"], k.H, k.W, k.stride, k.thr, c["depth"], c["depth_points"])
    assert gc.proj_error(out["z"][:, None], ref["z64"][:, None]) <= BAR
    if k.kind == "edge":
        assert np.array_equal(out["proj"], w["proj64"].astype(np.float32), equal_nan=True)
    M = (k.H // k.stride) * (k.W // k.stride)
    dense = np.zeros((k.N, M), dtype=np.int64)
    dense[w["pairs"][0], w["pairs"][1]] = 1     # the reference's formulation of conf_matrix_gt
    assert np.array_equal(_geom_lib.conf_target(dev(out["gt_j"]), M, torch.int64).cpu().numpy(), dense)


# ------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("N, V", [(1, 2), (63, 2), (64, 2), (65, 2), (255, 2), (256, 2), (257, 2), (SECOND_LEVEL, 2), (257, 1), (257, 64)])
def test_scan_and_emit_at_the_shapes_where_they_can_go_wrong(N, V):
    s = sweep(N, V)
    for dtype in (torch.float32, torch.float64):   # the fp64 pose is the widened fp32 one: the same result
        mask, idx, info = _geom_lib.select_visible(dev(s["pts"]), dev(s["poses"], dtype), dev(s["K"]), H, W)
        assert np.array_equal(mask.cpu().numpy(), s["vis"][0]) and np.array_equal(idx.cpu().numpy(), s["vis"][1]) and np.array_equal(info.cpu().numpy(), s["vis"][2])
        out = _geom_lib.build_pairs(dev(s["pts"]), dev(s["query"], dtype), dev(s["K"]), H, W, STRIDE, THR, dev(s["depth"]), True)
        same_pairs(host(out), s["pairs"])
    again = _geom_lib.build_pairs(dev(s["pts"]), dev(s["query"]), dev(s["K"]), H, W, STRIDE, THR, dev(s["depth"]), True)
    assert all(torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)) for k in out)   # two calls, the same bits


def test_depth_map_source_against_the_restatement():
    s = sweep(257, 2)
    depth = gc.sweep_depth(s["pts"], s["query"], s["K"], H, W, THR, 7, False)
    ref = gr.build_pairs(s["pts"], s["query"], s["K"], H, W, STRIDE, THR, depth, False)
    assert ref["pos"].sum() >= 4 and ref["valid"].sum() > ref["pos"].sum()
    same_pairs(host(_geom_lib.build_pairs(dev(s["pts"]), dev(s["query"]), dev(s["K"]), H, W, STRIDE, THR, dev(depth))), ref)
    for stride in (1, 16):   # other cell sizes
        same_pairs(host(_geom_lib.build_pairs(dev(s["pts"]), dev(s["query"]), dev(s["K"]), H, W, stride, THR, dev(depth))),
                   gr.build_pairs(s["pts"], s["query"], s["K"], H, W, stride, THR, depth, False))


@pytest.mark.parametrize("N", [257, SECOND_LEVEL])
def test_capacity_below_the_total_keeps_the_first_and_flags_overflow(N):
    s = sweep(N, 2)
    total_v, total_p = int(s["vis"][2][1]), int(s["pairs"]["info"][1])
    assert total_v > 5 and total_p > 5
    for cap in (1, 5, total_v, total_v + 3):
        ref = gr.select_visible(s["pts"], s["poses"], s["K"], H, W, cap)
        mask, idx, info = _geom_lib.select_visible(dev(s["pts"]), dev(s["poses"]), dev(s["K"]), H, W, cap)
        assert idx.shape == (cap,) and np.array_equal(idx.cpu().numpy(), ref[1]) and np.array_equal(info.cpu().numpy(), ref[2])
        assert info[2].item() == (cap < total_v) and not idx[total_v:].any() and np.array_equal(mask.cpu().numpy(), ref[0])
    for cap in (1, 5, total_p, total_p + 3):
        ref = gr.build_pairs(s["pts"], s["query"], s["K"], H, W, STRIDE, THR, s["depth"], True, cap)
        out = host(_geom_lib.build_pairs(dev(s["pts"]), dev(s["query"]), dev(s["K"]), H, W, STRIDE, THR, dev(s["depth"]), True, cap))
        same_pairs(out, ref)
        assert out["pairs"].shape == (2, cap) and out["info"][2] == (cap < total_p) and not out["pairs"][:, total_p:].any()


def test_a_rows_result_does_not_depend_on_the_other_rows():
    s = sweep(257, 2)
    full = host(_geom_lib.build_pairs(dev(s["pts"]), dev(s["query"]), dev(s["K"]), H, W, STRIDE, THR, dev(s["depth"]), True))
    fmask = _geom_lib.select_visible(dev(s["pts"]), dev(s["poses"]), dev(s["K"]), H, W)[0].cpu().numpy()
    rows = np.arange(3, 257, 5)
    part = host(_geom_lib.build_pairs(dev(s["pts"][rows]), dev(s["query"]), dev(s["K"]), H, W, STRIDE, THR, dev(s["depth"][rows]), True))
    for k in ("proj", "z", "valid", "pos"):
        assert np.array_equal(part[k], full[k][rows], equal_nan=True), k
    assert np.array_equal(_geom_lib.select_visible(dev(s["pts"][rows]), dev(s["poses"]), dev(s["K"]), H, W)[0].cpu().numpy(), fmask[rows])


# ------------------------------------------------------------------------------------------ the target and the grid
def _gt(N, M, seed):
    """gt_j with -1, 0, M - 1 and M (ignored) among random cells."""
    g = np.random.default_rng(seed).integers(-1, M + 1, size=N).astype(np.int32)
    g[:4] = [-1, 0, M - 1, M]
    return g


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 4800])
def test_conf_target_writes_every_value_once(M, dtype):
    N = 7   # odd: with M = 3, 5 rows start off the 16-byte grid
    g = _gt(N, M, M)
    npdt = np.float32 if dtype == torch.float32 else np.int64
    want = gr.conf_target(g, M, npdt)
    out = _geom_lib.conf_target(dev(g), M, dtype)
    assert out.dtype == dtype and np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(out, _geom_lib.conf_target(dev(g), M, dtype))
    for rows in ((2, 5), (6, 7), (0, 1), (3, 3)):   # a slice: values before and after the aligned part
        assert np.array_equal(_geom_lib.conf_target(dev(g), M, dtype, rows).cpu().numpy(), want[rows[0]:rows[1]])
    # a destination off the 16-byte grid (the scalar path), with a guard value on either side
    es = 4 if dtype == torch.float32 else 8
    buf = torch.full((N * M + 2,), 7, dtype=dtype, device="cuda")
    st = _geom_lib.load().nlg_conf_target(dev(g).data_ptr(), N, M, _geom_lib.TARGET_F32 if es == 4 else _geom_lib.TARGET_I64, 0, N, buf.data_ptr() + es,
                                          _lib.stream(buf.device))
    assert st == _lib.NL_OK and buf[0].item() == 7 and buf[-1].item() == 7 and np.array_equal(buf[1:-1].cpu().numpy().reshape(N, M), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
def test_conf_target_indexes_past_2_to_the_31_on_a_row_subset(dtype):
    N, M = 1 << 20, 4800   # 5.03e9 values: never allocated
    g = np.full(N, -1, dtype=np.int32)
    cross = (1 << 31) // M   # the row in which element index 2^31 lies
    picks = {cross - 1: 0, cross: M - 1, cross + 1: 17, N - 2: 4799, N - 1: 0}
    for r, j in picks.items():
        g[r] = j
    gd = dev(g)
    for rows in ((cross - 1, cross + 2), (N - 3, N)):
        assert rows[1] * M > 1 << 31
        out = _geom_lib.conf_target(gd, M, dtype, rows).cpu().numpy()
        assert out.shape == (3, M) and np.array_equal(out, gr.conf_target(g, M, out.dtype, rows))
        assert out.sum() == sum(1 for r in picks if rows[0] <= r < rows[1])


def test_cell_grid_against_arange():
    for Hc, Wc, scale in ((6, 8, 1.0), (3, 5, 4.0), (1, 1, 2.0), (60, 80, 4.0)):
        want = torch.stack([torch.arange(Wc).repeat(Hc), torch.arange(Hc).repeat_interleave(Wc)], dim=1).float() * scale
        out = _geom_lib.cell_grid(Hc, Wc, scale)
        assert torch.equal(out.cpu(), want) and np.array_equal(out.cpu().numpy(), gr.cell_grid(Hc, Wc, scale))
    buf = torch.full((2 * 15 + 4,), -1.0, device="cuda")   # 8-byte aligned only: scalar stores
    assert _geom_lib.load().nlg_cell_grid(3, 5, 1.0, buf.data_ptr() + 8, _lib.stream(buf.device)) == _lib.NL_OK
    assert buf[:2].tolist() == [-1.0, -1.0] and buf[-2:].tolist() == [-1.0, -1.0] and np.array_equal(buf[2:-2].cpu().numpy().reshape(15, 2), gr.cell_grid(3, 5))
    a, b = kp.cell_grid(6, 8, 4.0, "cuda"), kp.cell_grid(6, 8, 4.0, "cuda")
    assert a is b and kp.pts2d_grid(48, 64, 8, "cuda").dtype == torch.int64   # the per-(shape, device) cache


# ------------------------------------------------------------------------------------------ the drop-ins
def test_drop_ins_equal_the_eager_formulation_on_hip_tensors():
    for name in ("small", "views10", "depth_points", "fallback"):
        c, k = case(name), case(name)["case"]
        pts, poses, K, query, depth = dev(c["pts"]), dev(c["poses"]), dev(c["K"]), dev(c["query"]), dev(c["depth"])
        idx = kp.select_3d_keypoints(pts, list(poses), K, k.H, k.W)
        e_idx, e_mask = kp.eager_select_3d_keypoints(pts, poses, K, k.H, k.W)
        assert idx.dtype == torch.int64 and torch.equal(idx, e_idx) and torch.equal(kp.select_3d_keypoints(pts, poses.double(), K, k.H, k.W), e_idx)
        kw = {"depth_points": depth} if c["depth_points"] else {"depth_map": depth}
        same, grid, proj, pairs = kp.build_3d_2d_pairs(pts, k.H, k.W, K, query, k.thr, k.stride, **kw)
        e = kp.eager_build_3d_2d_pairs(pts, k.H, k.W, K, query, k.thr, k.stride, **kw)
        assert same is pts and torch.equal(pairs, e["pairs"]) and torch.equal(grid, kp.eager_cell_grid(k.H // k.stride, k.W // k.stride, 1.0, "cuda").long())
        assert gc.proj_error(proj.cpu().numpy(), e["proj"].double().cpu().numpy()) <= BAR
        out = kp.build_3d_2d_pairs_padded(pts, k.H, k.W, K, query, k.thr, k.stride, **kw)
        assert torch.equal(out["gt_j"], e["gt_j"]) and torch.equal(out["valid"], e["valid"]) and int(out["used_fallback"]) == int(e["used_fallback"])
        M = (k.H // k.stride) * (k.W // k.stride)
        for dtype in (torch.float32, torch.int64):
            assert torch.equal(kp.conf_matrix_target(out["gt_j"], M, dtype), kp.eager_conf_matrix_target(out["gt_j"], M, dtype))


def test_hip_tensors_of_an_unsupported_dtype_raise():
    c, k = case("small"), case("small")["case"]
    pts, poses, K = dev(c["pts"]), dev(c["poses"]), dev(c["K"])
    with pytest.raises(ValueError, match="fp32"):
        kp.select_3d_keypoints(pts.double(), poses, K, k.H, k.W)
    with pytest.raises(ValueError, match="fp32"):
        kp.build_3d_2d_pairs(pts, k.H, k.W, K.double(), dev(c["query"]), k.thr, k.stride, depth_map=dev(c["depth"]))
    with pytest.raises(ValueError, match="poses"):
        kp.select_3d_keypoints(pts, poses.half(), K, k.H, k.W)
    with pytest.raises(ValueError, match="int32"):
        kp.conf_matrix_target(torch.zeros(4, dtype=torch.int64, device="cuda"), 8)
    with pytest.raises(ValueError, match="one device"):
        kp.select_3d_keypoints(pts, poses.cpu(), K, k.H, k.W)


def test_padded_forms_replay_from_a_graph_with_new_inputs():
    a, b = case("small"), case("nonrigid")   # two recipes of one image size; the second is copied into the first's buffers
    k = a["case"]
    n = min(a["case"].N, b["case"].N)
    pts, poses, K, query, depth = dev(a["pts"][:n]), dev(a["poses"], torch.float64), dev(a["K"]), dev(a["query"], torch.float64), dev(a["depth"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: the libraries load here
        kp.select_3d_keypoints_padded(pts, poses, K, k.H, k.W, capacity=64)
        kp.build_3d_2d_pairs_padded(pts, k.H, k.W, K, query, k.thr, k.stride, depth_map=depth, capacity=64)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # a synchronisation or a host read in here would fail the capture
        idx, mask, num, overflow = kp.select_3d_keypoints_padded(pts, poses, K, k.H, k.W, capacity=64)
        out = kp.build_3d_2d_pairs_padded(pts, k.H, k.W, K, query, k.thr, k.stride, depth_map=depth, capacity=64)
        target = kp.conf_matrix_target(out["gt_j"], (k.H // k.stride) * (k.W // k.stride))
    for c in (a, b):
        pts.copy_(dev(c["pts"][:n])), poses.copy_(dev(c["poses"], torch.float64)), query.copy_(dev(c["query"], torch.float64)), depth.copy_(dev(c["depth"]))
        graph.replay()
        torch.cuda.synchronize()
        ref_v = gr.select_visible(c["pts"][:n], c["poses"], c["K"], k.H, k.W, 64)
        ref_p = gr.build_pairs(c["pts"][:n], c["query"], c["K"], k.H, k.W, k.stride, k.thr, c["depth"], False, 64)
        assert np.array_equal(idx.cpu().numpy(), ref_v[1]) and [int(num), int(overflow)] == [ref_v[2][0], ref_v[2][2]] and np.array_equal(mask.cpu().numpy(), ref_v[0])
        assert np.array_equal(out["pairs"].cpu().numpy(), ref_p["pairs"]) and np.array_equal(out["gt_j"].cpu().numpy(), ref_p["gt_j"])
        assert [int(out["num"]), int(out["overflow"]), int(out["used_fallback"])] == ref_p["info"][[0, 2, 3]].tolist()
        assert np.array_equal(target.cpu().numpy(), gr.conf_target(ref_p["gt_j"], target.shape[1]))


def test_fp32_target_gives_s2d_training_the_same_bits_as_the_dense_int64_tensor():
    N, M, C = 64, 160, 64
    rng = np.random.default_rng(5)
    gt = rng.integers(-1, M, size=N).astype(np.int32)
    d0, d1 = (0.3 * rng.standard_normal((N, C))).astype(np.float32), (0.3 * rng.standard_normal((M, C))).astype(np.float32)
    torch.manual_seed(3)
    mod = S2DMatching(C).to("cuda").train()
    rows = torch.nonzero(dev(gt) >= 0).squeeze(1)
    dense = torch.zeros([N, M], device="cuda").long()   # the reference's way: zeros().long() and an index-put of the pairs
    dense[rows, dev(gt)[rows].long()] = 1
    target = kp.conf_matrix_target(dev(gt), M, torch.float32)
    assert target.dtype == torch.float32 and target.to(torch.float32).data_ptr() == target.data_ptr() and torch.equal(target, dense.float())
    results = []
    for tgt in (dense, target):
        a, b = dev(d0).requires_grad_(True), dev(d1).requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        data = mod(a, b, {"conf_matrix_gt": tgt})
        data["coarse_loss"].backward()
        results.append([data["coarse_loss"].detach(), a.grad, b.grad] + [p.grad for p in mod.parameters()])
    assert float(results[0][0]) > 0
    for x, y in zip(*results):
        assert torch.equal(x, y)
