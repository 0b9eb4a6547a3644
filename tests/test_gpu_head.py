"""GPU tests of the localisation head as one object: the entry points of libnerfloc_head.so (csrc/head.hip, csrc/head_pnp.hip) against their numpy restatement
(tests/head_ref.py) and against nl_pnp_ransac, and nerf_loc_amd/matcher.py — `forward` against the reference's goldens (tests/golden/head_*.npz), `forward_padded`
and `localize` against `forward` + pose.absolute_pose bit for bit, and `localize` replayed from a captured graph.  Errors are max |a - b| / max |b| with b the
reference; the bar is the project's 1e-4 (the goldens carry the reference's own fp32-versus-fp64 deviation: at most 1.5e-5, on the C = 192 position tables)."""
import ctypes as ct
import functools
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _head_lib, _lib, pose
from nerf_loc_amd.position_encoding import PositionEmbeddingSine, get_embedder
from tests import head_cases as hc
from tests import head_ref as hr
from tests import pnp_cases as pc
from tests.test_head_cpu import BAR, build_matcher, case, golden, rel, tensors, zero_dropout

pytestmark = pytest.mark.gpu


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ nlh_select_matches
def lib_select(match_j, cap, Mc, kps3d, kps2d, rows_a=None, rows_b=None):
    """The library call on poisoned output buffers (ids -7, floats NaN), so that a padded row that is not written shows."""
    lib = _head_lib.load()
    N = len(match_j)
    C = rows_a.shape[1] if rows_a is not None else rows_b.shape[1] if rows_b is not None else 0
    mj, k3, k2 = _dev(match_j.astype(np.int32)), _dev(kps3d), _dev(kps2d)
    ra, rb = (None if r is None else _dev(r) for r in (rows_a, rows_b))
    ids = torch.full((3, cap), -7, dtype=torch.int64, device="cuda")
    mk3 = torch.full((cap, 3), float("nan"), device="cuda")
    mk2 = torch.full((cap, 2), float("nan"), device="cuda")
    oa, ob = (None if r is None else torch.full((cap, C), float("nan"), device="cuda") for r in (rows_a, rows_b))
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    need = lib.nlh_select_workspace_bytes(N)
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = _lib.ptr
    st = lib.nlh_select_matches(mj.data_ptr(), N, cap, Mc, C, k3.data_ptr(), k2.data_ptr(), ptr(ra), ptr(rb), ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(),
                                mk3.data_ptr(), mk2.data_ptr(), ptr(oa), ptr(ob), info.data_ptr(), ws.data_ptr(), need, _st())
    assert st == _lib.NL_OK, st
    out = {"i_ids": ids[0], "j_ids": ids[1], "b_ids": ids[2], "mkps3d": mk3, "mkps2d_c": mk2, "out_a": oa, "out_b": ob, "info": info}
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _same_selection(got, want):
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == w.dtype and np.array_equal(got[k].view(np.uint8), w.view(np.uint8)), k   # bytes: -0.0 and NaN would show


def _match_pattern(kind, N, Mc, rng):
    if kind == "none":
        return np.full(N, -1, dtype=np.int32)
    if kind == "all":
        return rng.integers(0, Mc, size=N).astype(np.int32)
    mj = np.where(rng.uniform(size=N) < 0.6, rng.integers(0, Mc, size=N), -1).astype(np.int32)
    bad = rng.permutation(N)[:max(N // 8, 1)]
    mj[bad] = rng.choice(np.array([Mc, Mc + 5, -2, np.iinfo(np.int32).max, np.iinfo(np.int32).min], dtype=np.int64), size=len(bad)).astype(np.int32)   # unmatched, never read through
    return mj


@pytest.mark.parametrize("N", (1, 63, 64, 65, 1100))
def test_select_matches_equals_the_restatement_exactly(N):
    rng = np.random.default_rng(300 + N)
    Mc, C = 37, 192 if N == 65 else 8
    kps3d = rng.standard_normal((N, 3)).astype(np.float32)
    kps2d = rng.standard_normal((Mc, 2)).astype(np.float32)
    ra, rb = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    seen = set()
    for kind in ("none", "all", "mixed"):
        mj = _match_pattern(kind, N, Mc, rng)
        total = int(((mj >= 0) & (mj < Mc)).sum())
        assert total == {"none": 0, "all": N}.get(kind, total)
        for cap in sorted({max(total - 2, 1), max(total, 1), total + 3, N, 1}):
            want = hr.select_matches(mj, cap, Mc, kps3d, kps2d, ra, rb)
            assert want["info"].tolist() == [min(total, cap), total, int(total > cap), 0]
            seen.add((int(want["info"][2]), bool(want["info"][0] < cap)))
            got = lib_select(mj, cap, Mc, kps3d, kps2d, ra, rb)
            _same_selection(got, want)
            k = int(want["info"][0])
            assert not got["out_a"][k:].any() and not got["mkps3d"][k:].any() and not got["i_ids"][k:].any() and (np.diff(got["i_ids"][:k]) > 0).all()
        # NULL row tables, one and both; two calls give the same bits
        cap = max(total, 1)
        _same_selection(lib_select(mj, cap, Mc, kps3d, kps2d, None, rb), hr.select_matches(mj, cap, Mc, kps3d, kps2d, None, rb))
        a, b = lib_select(mj, cap, Mc, kps3d, kps2d), lib_select(mj, cap, Mc, kps3d, kps2d)
        _same_selection(a, hr.select_matches(mj, cap, Mc, kps3d, kps2d))
        _same_selection(a, b)
    if N > 1:
        assert seen == {(0, False), (0, True), (1, False)}   # exact fit, padded rows, overflow: all met


def test_select_matches_module_wrapper_and_large_n():
    """_head_lib.select_matches (what Matcher calls), at the largest N the entry point takes: more than one chunk per thread of the scan."""
    rng = np.random.default_rng(7)
    N, Mc = 1 << 20, 4800
    mj = np.where(rng.uniform(size=N) < 0.01, rng.integers(0, Mc, size=N), -1).astype(np.int32)
    kps3d, kps2d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((Mc, 2)).astype(np.float32)
    want = hr.select_matches(mj, 4096, Mc, kps3d, kps2d)
    got = _head_lib.select_matches(_dev(mj), 4096, _dev(kps3d), _dev(kps2d))
    assert want["info"][2] == 1 and got["out_a"] is None
    for k in ("i_ids", "j_ids", "b_ids", "mkps3d", "mkps2d_c", "info"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


# ------------------------------------------------------------------------------------------ position encodings
@pytest.mark.parametrize("C", hc.POS_CHANNELS)
def test_position_tables_meet_the_reference(C):
    g = golden(f"pos_c{C}")
    mod = PositionEmbeddingSine(C // 2, normalize=True, sine_type="lin_sine")
    for H, W in hc.POS_SHAPES:
        out = mod(torch.zeros(3, H, W, device="cuda"))
        assert tuple(out.shape) == (3, H, W, C) and out.is_cuda and out.dtype == torch.float32
        assert out.stride(0) == 0 and mod(torch.zeros(1, H, W, device="cuda")).data_ptr() == out.data_ptr()   # the cached table, expanded: no copy, no launch
        err = rel(out[2].cpu().numpy(), g[f"pos_{H}x{W}"])
        print(f"pos {H}x{W} C {C}: {err:.2e}")
        assert err <= BAR
        again = _head_lib.pos_sine_grid(H, W, C, torch.device("cuda", 0))
        assert torch.equal(again, out[0])


@pytest.mark.parametrize("n", (1, 65))
def test_embedder_meets_the_reference_at_full_range(n):
    """L = 32: arguments up to 2^31 |x|.  A fast hardware sine is wrong by O(1) there; the bar is 1e-4 of the table's scale (1)."""
    g = golden("embed")
    fn, dim = get_embedder(hc.EMBED_L, 0, include_input=False)
    x = hc.embed_points_input(n)
    out = fn(_dev(x))
    assert tuple(out.shape) == (n, dim) and dim == 192 and out.is_cuda
    got = out.cpu().numpy()
    err32, err64 = rel(got, g[f"embed_{n}"]), rel(got, g[f"embed64_{n}"])
    high = rel(got[:, 180:], g[f"embed_{n}"][:, 180:])   # the two highest frequencies alone
    print(f"embed N {n}: vs reference fp32 {err32:.2e}, fp64 {err64:.2e}; frequencies 2^30, 2^31: {high:.2e}")
    assert err32 <= BAR and err64 <= BAR and high <= BAR
    assert torch.equal(fn(_dev(x)), out)
    assert tuple(fn(_dev(x).reshape(n, 1, 3)).shape) == (n, 1, dim)


# ------------------------------------------------------------------------------------------ nlh_pnp_ransac_counted
def _ransac(problems, H, counts=None, seed=0, min_inliers=4):
    """problems: [(pts2d, pts3d, K, thr)].  counts None: nl_pnp_ransac; else nlh_pnp_ransac_counted with these device counts (the problems' sizes = capacities)."""
    B = len(problems)
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in problems])]).astype(np.int64)
    Mt = int(off[-1])
    d2 = _dev(np.concatenate([p[0].reshape(-1, 2) for p in problems]).astype(np.float32)) if Mt else None
    d3 = _dev(np.concatenate([p[1].reshape(-1, 3) for p in problems]).astype(np.float32)) if Mt else None
    posed = torch.full((B, 12), float("nan"), dtype=torch.float64, device="cuda")
    mask = torch.full((max(Mt, 1),), 9, dtype=torch.uint8, device="cuda")
    info = torch.full((B, 4), -7, dtype=torch.int32, device="cuda")
    cnts = torch.full((B, 4 * H), -7, dtype=torch.int32, device="cuda")
    offs = (ct.c_int32 * (B + 1))(*off.tolist())
    intr = (ct.c_double * (4 * B))(*[v for p in problems for v in p[2]])
    thr = (ct.c_double * B)(*[float(p[3]) for p in problems])
    ptr = _lib.ptr
    if counts is None:
        lib = _lib.load()
        need = lib.nl_pnp_workspace_bytes(Mt, B, H)
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
        st = lib.nl_pnp_ransac(ptr(d2), ptr(d3), offs, intr, thr, B, H, seed, min_inliers, posed.data_ptr(), mask.data_ptr() if Mt else None, info.data_ptr(),
                               cnts.data_ptr(), ws.data_ptr(), need, _st())
    else:
        lib = _head_lib.load()
        need = lib.nlh_pnp_workspace_bytes(Mt, B, H)
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
        cd = _dev(np.asarray(counts, dtype=np.int32))
        st = lib.nlh_pnp_ransac_counted(ptr(d2), ptr(d3), offs, cd.data_ptr(), intr, thr, B, H, seed, min_inliers, posed.data_ptr(), mask.data_ptr() if Mt else None,
                                        info.data_ptr(), cnts.data_ptr(), ws.data_ptr(), need, _st())
    assert st == _lib.NL_OK and need > 0, st
    posed, mask, info, cnts = posed.cpu().numpy(), mask.cpu().numpy(), info.cpu().numpy(), cnts.cpu().numpy()
    return [{"pose": posed[b], "mask": mask[off[b]:off[b + 1]], "info": info[b], "counts": cnts[b]} for b in range(B)]


def _same_pose(counted, plain, c):
    assert np.array_equal(counted["pose"].view(np.uint64), plain["pose"].view(np.uint64)) and np.array_equal(counted["info"], plain["info"])
    assert np.array_equal(counted["counts"], plain["counts"])
    assert np.array_equal(counted["mask"][:c], plain["mask"]) and not counted["mask"][c:].any()


@functools.lru_cache(maxsize=None)
def scene(name):
    return pc.make_case(name)


def _problem(name, c=None, thr=None):
    s = scene(name)
    return (s["pts2d"][:c], s["pts3d"][:c], pc.K, s["case"].thr if thr is None else thr)


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_counted_with_the_capacity_gives_the_bits_of_nl_pnp_ransac(name):
    c = pc.CASES[name]
    plain = _ransac([_problem(name)], c.H)[0]
    assert plain["info"][0] == 1
    _same_pose(_ransac([_problem(name)], c.H, counts=[c.M])[0], plain, c.M)
    _same_pose(_ransac([_problem(name)], c.H, counts=[c.M + 1000])[0], plain, c.M)   # a count above the capacity is the capacity


@pytest.mark.parametrize("count", (0, 3, 4, 65, 255, -4))
def test_counted_below_the_capacity_gives_the_bits_of_the_first_matches(count):
    """`half`: capacity 256.  The restated call is nl_pnp_ransac on the first c matches; mask bytes at and beyond c are 0 (the buffer is poisoned with 9)."""
    H = pc.CASES["half"].H
    c = max(count, 0)
    plain = _ransac([_problem("half", c)], H)[0]
    counted = _ransac([_problem("half")], H, counts=[count])[0]
    _same_pose(counted, plain, c)
    if c < 4:
        assert counted["info"].tolist() == [0, 0, 0, -1] and counted["pose"].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]   # a failure, not an error
    elif c >= 65:
        assert counted["info"][0] == 1   # half of the scene's matches are inliers of its pose


def test_counted_problems_of_a_batch_equal_their_solo_calls():
    names, counts, thrs = ("clean65", "half", "tight"), (40, 100, 299), (8.0, 4.0, 2.0)
    probs = [_problem(n, thr=t) for n, t in zip(names, thrs)]
    empty = (np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32), pc.K, 1.0)
    both = _ransac(probs, 64, counts=counts)
    for b in range(3):
        solo = _ransac([empty] * b + [_problem(names[b], counts[b], thrs[b])], 64)[b]    # problem b draws the samples of index b
        _same_pose(both[b], solo, counts[b])
        assert both[b]["info"][0] == 1
    again = _ransac(probs, 64, counts=counts)
    for a, b in zip(again, both):
        _same_pose(a, b, len(b["mask"]))
    # 17 problems: more than one launch per kernel, the counts indexed across the launches
    many = _ransac([probs[i % 3] for i in range(17)], 64, counts=[counts[i % 3] for i in range(17)])
    _same_pose(many[0], both[0], len(both[0]["mask"]))
    _same_pose(many[16], _ransac([empty] * 16 + [_problem(names[1], counts[1], thrs[1])], 64)[16], counts[1])


# ------------------------------------------------------------------------------------------ Matcher.forward against the reference
@functools.lru_cache(maxsize=None)
def eval_run(name, precision):
    m = build_matcher(name, precision=precision).cuda().eval()
    with torch.no_grad():
        out = m(tensors(case(name)["data"], "cuda"))
    return m, out


@pytest.mark.parametrize("precision", ("fp32", "bf16x3"))
@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_forward_in_eval_mode_meets_the_reference(name, precision):
    g = golden(name)
    _, out = eval_run(name, precision)
    assert sorted(set(out) - set(case(name)["data"])) == g["eval_keys"].tolist()
    for k in ("i_ids", "j_ids", "b_ids"):
        assert out[k].dtype == torch.int64 and np.array_equal(out[k].cpu().numpy(), g[k]), k     # the reference's pairs exactly, no exclusions
    assert torch.equal(out["pairs"][0], out["i_ids"]) and torch.equal(out["pairs"][1], out["j_ids"])
    assert np.array_equal(out["mkps3d"].cpu().numpy(), g["mkps3d"]) and np.array_equal(out["mkps2d_c"].cpu().numpy(), g["mkps2d_c"])
    for k in ("score_matrix", "expec_f", "mkps2d_f"):
        err = rel(out[k].cpu().numpy(), g[k])
        print(f"{name} {precision} {k}: {err:.2e} (reference fp32 vs fp64 {float(g['dev_' + k]):.1e})")
        assert tuple(out[k].shape) == g[k].shape and err <= BAR, k


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_forward_branches_return_the_reference_keys_and_shapes(name):
    g = golden(name)
    data = case(name)["data"]

    def shapes(out, keys):
        return [",".join(str(s) for s in out[k].shape) if torch.is_tensor(out[k]) else type(out[k]).__name__ for k in keys]
    m = build_matcher(name).cuda().eval()
    m.coarse_matcher.thr = 2.0   # no score reaches it: the M == 0 branch
    with torch.no_grad():
        out = m(tensors(data, "cuda"))
    keys = sorted(set(out) - set(data))
    assert keys == g["m0_keys"].tolist() and shapes(out, keys) == g["m0_shapes"].tolist() and len(out["i_ids"]) == 0
    coarse = build_matcher(name, fine_matching=False).cuda().eval()
    with torch.no_grad():
        out = coarse(tensors(data, "cuda"))
    keys = sorted(set(out) - set(data))
    assert keys == g["nofine_keys"].tolist() and shapes(out, keys) == g["nofine_shapes"].tolist() and np.array_equal(out["i_ids"].cpu().numpy(), g["i_ids"])


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_forward_in_training_mode_meets_the_reference(name):
    c = case(name)
    with np.load(os.path.join(hc.golden_dir(), f"head_{name}_train.npz")) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(hc.golden_dir(), f"head_{name}_train_map.npz")) as z:
        g["grad_feat_fine"] = z["grad_feat_fine"]
    m = zero_dropout(build_matcher(name)).cuda().train()
    data = tensors(c["data"], "cuda", grads=hc.INPUT_GRADS)
    out = m(data)
    assert sorted(set(out) - set(c["data"])) == g["train_keys"].tolist()
    (out["coarse_loss"] + out["fine_loss"]).backward()
    for k in ("coarse_loss", "fine_loss", "fine_err"):
        err = abs(out[k].item() - float(g[k + "_64"])) / abs(float(g[k + "_64"]))
        print(f"{name} {k}: {err:.2e}")
        assert err <= BAR, k
    for k in hc.INPUT_GRADS:
        err = rel(data[k].grad.cpu().numpy(), g["grad_" + k])
        print(f"{name} grad {k}: {err:.2e}")
        assert err <= BAR, k


# ------------------------------------------------------------------------------------------ forward_padded and localize
PADDED_KEYS = ("i_ids", "j_ids", "b_ids", "mkps3d", "mkps2d_c", "expec_f", "mkps2d_f")
IMAGE_K = (100.0, 100.0, 40.0, 30.0)
POSE_THR = 24.0   # pixels: a planted pair is off by at most 3 fine cells x stride_fine = 12 px per axis (17 px) under the scene's pose


def geometric_kps3d(name):
    """kps3d such that every planted pair satisfies one camera pose: the 3-D point of row i projects onto its partner's cell (in pixels: kps2d x stride_fine)."""
    c = case(name)
    rng = np.random.default_rng(5)
    R, t = pc.rodrigues(0.3 * rng.normal(size=3)), np.array([0.1, -0.2, 0.3])
    N = c["case"].N
    px = rng.uniform(0, 60, size=(N, 2))
    ok = c["planted"] >= 0
    px[ok] = c["data"]["kps2d"][c["planted"][ok]] * hc.STRIDE_FINE
    depth = rng.uniform(2.0, 8.0, size=N)
    cam = np.stack([(px[:, 0] - IMAGE_K[2]) / IMAGE_K[0] * depth, (px[:, 1] - IMAGE_K[3]) / IMAGE_K[1] * depth, depth], axis=1)
    return ((cam - t) @ R).astype(np.float32)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.reshape(-1).contiguous().view(torch.uint8) == b.reshape(-1).contiguous().view(torch.uint8)).all())


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_forward_padded_equals_forward_bit_for_bit(name):
    m, ref = eval_run(name, "bf16x3")
    data = tensors(case(name)["data"], "cuda")
    M, N = len(ref["i_ids"]), case(name)["case"].N
    for cap in (None, M, M - 5):
        out = m.forward_padded(data, cap)
        rows = N if cap is None else cap
        k = min(M, rows)
        assert int(out["num_matches"]) == k and int(out["overflow"]) == int(M > rows) and out["num_matches"].is_cuda and "num_matches" not in data
        for key in PADDED_KEYS:
            assert out[key].shape[0] == rows and _bits(out[key][:k], ref[key][:k]), (cap, key)
            assert bool(torch.isfinite(out[key].float()).all()), key     # padded rows are computed and finite
        assert _bits(out["score_matrix"], ref["score_matrix"]) and not out["i_ids"][k:].any() and not out["mkps3d"][k:].any()
    m.coarse_matcher.thr = 2.0
    try:
        out = m.forward_padded(data)
        assert int(out["num_matches"]) == 0 and not out["i_ids"].any() and bool(torch.isfinite(out["expec_f"]).all())
    finally:
        m.coarse_matcher.thr = hc.THR


@functools.lru_cache(maxsize=None)
def localize_run(name):
    m, _ = eval_run(name, "bf16x3")
    data = tensors(case(name)["data"], "cuda")
    data["kps3d"] = _dev(geometric_kps3d(name))
    with torch.no_grad():
        ref = m(dict(data))
    want = pose.absolute_pose(ref["mkps2d_f"] * data["stride_fine"], ref["mkps3d"], IMAGE_K, POSE_THR, hypotheses=256, seed=3)
    got = m.localize(data, IMAGE_K, POSE_THR, hypotheses=256, seed=3)
    return m, data, ref, want, got


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_localize_equals_absolute_pose_on_the_matches_of_forward(name):
    m, data, ref, want, got = localize_run(name)
    M, N = len(ref["i_ids"]), case(name)["case"].N
    assert int(got["num_matches"]) == M and int(got["overflow"]) == 0
    for k in ("T_w2c", "T_c2w", "num_inliers", "success", "best_candidate", "best_count"):
        assert _bits(got[k], want[k]), k
    assert got["inliers"].dtype == torch.bool and tuple(got["inliers"].shape) == (N,) and torch.equal(got["inliers"][:M], want["inliers"]) and not got["inliers"][M:].any()
    assert got["T_w2c"].dtype == torch.float64 and tuple(got["T_w2c"].shape) == (4, 4)
    print(f"{name}: {M} matches, {int(got['num_inliers'])} inliers, success {int(got['success'])}")
    # the planted pairs satisfy one pose within POSE_THR by construction
    assert int(got["success"]) == 1 and int(got["num_inliers"]) >= 8
    # a smaller capacity: the first rows, overflow set; the solver sees those rows alone
    small = m.localize(data, IMAGE_K, POSE_THR, hypotheses=256, seed=3, capacity=M - 5)
    cut = pose.absolute_pose(ref["mkps2d_f"][:M - 5] * data["stride_fine"], ref["mkps3d"][:M - 5], IMAGE_K, POSE_THR, hypotheses=256, seed=3)
    assert int(small["overflow"]) == 1 and int(small["num_matches"]) == M - 5 and _bits(small["T_w2c"], cut["T_w2c"]) and torch.equal(small["inliers"], cut["inliers"])


def test_localize_without_a_match_gives_the_identity_and_no_error():
    m, data, _, _, _ = localize_run("head64")
    m.coarse_matcher.thr = 2.0   # every score is below it
    try:
        got = m.localize(data, IMAGE_K, POSE_THR, hypotheses=64)
    finally:
        m.coarse_matcher.thr = hc.THR
    assert int(got["num_matches"]) == 0 and int(got["success"]) == 0 and int(got["num_inliers"]) == 0 and not got["inliers"].any()
    assert torch.equal(got["T_w2c"], torch.eye(4, dtype=torch.float64, device="cuda")) and torch.equal(got["T_c2w"], got["T_w2c"])


def test_localize_replays_from_a_captured_graph():
    """One capture after a warm call; two replays with other descriptors copied into the static inputs; each equals the eager call's bits.  A host synchronisation
    or an allocation outside torch's allocator during the capture would be an error, so the captured call made none."""
    m, data, _, _, first = localize_run("head64")
    keys = ("T_w2c", "T_c2w", "inliers", "num_inliers", "success", "num_matches", "overflow", "i_ids", "j_ids", "mkps3d", "mkps2d_f", "expec_f")
    variants = []
    for shift in (7, 0):   # other descriptors: the 3-D rows rolled (other pairs, another order), then the recipe's own
        d3 = torch.roll(data["desc_3d"], shift, 0).clone()
        eager = m.localize({**data, "desc_3d": d3}, IMAGE_K, POSE_THR, hypotheses=256, seed=3)
        variants.append((d3, {k: eager[k].clone() for k in keys}))
    assert all(_bits(variants[1][1][k], first[k]) for k in keys)
    assert not torch.equal(variants[0][1]["i_ids"], variants[1][1]["i_ids"])
    static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = m.localize(static, IMAGE_K, POSE_THR, hypotheses=256, seed=3)
    for d3, eager in variants:
        for k in keys:
            cap[k].zero_()
        static["desc_3d"].copy_(d3)
        g.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert _bits(cap[k], eager[k]), k
