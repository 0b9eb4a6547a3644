"""GPU tests of the counted matcher (libnerfloc_counted.so, nerf_loc_amd/cascade.py).  Everywhere the truth is the exact-size path on the truncated or gathered
inputs — nl_sct_layer, nl_sct_forward, nl_s2d_match, Matcher.forward with pose.absolute_pose, keypoints.select_3d_keypoints — which the existing tests pin to the
reference's goldens, and the bar is bit equality.  The rows behind the count hold adversarial finite values (copies of valid rows, of the rows with planted
partners where there are such, scaled by 8): unmasked they would win column maxima and shift every softmax, and each test first shows that the un-counted call on
the same padded inputs gives another result."""
import functools

import numpy as np
import pytest
import torch

from nerf_loc_amd import _counted_lib, _lib, cascade, keypoints, pose
from nerf_loc_amd.matching import S2DMatching
from nerf_loc_amd.transformer import SelfCrossTransformer
from tests import counted_ref as cr
from tests import head_cases as hc
from tests import match_cases as mc
from tests import pnp_cases as pc
from tests import sct_cases as sc
from tests.test_head_cpu import build_matcher, case, tensors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("fp32", "bf16x3")
C, F = 64, 64
CAP = 544                                                   # 17 key tiles: four ranges
COUNTS = (1, 31, 32, 33, 96, 97, 128, 480, 481, 544)        # both sides of every tile boundary met and of both range thresholds (4 and 16 tiles)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.reshape(-1).contiguous().view(torch.uint8) == b.reshape(-1).contiguous().view(torch.uint8)).all())


def _cnt(n):
    return torch.tensor(int(n), dtype=torch.int32, device=DEV)


def _finite(t):
    return bool(torch.isfinite(t.double()).all())


def _pad_rows(x, n, scale=8.0, src=None):
    """x (.., N, C) with the rows at and beyond n replaced by scaled copies of rows below n (src: the candidate rows; default all of them), cycling."""
    N = x.shape[-2]
    out = x.clone()
    if n < N:
        pool = torch.arange(max(n, 1), device=x.device) if src is None else src
        out[..., n:, :] = scale * x[..., pool[torch.arange(N - n, device=x.device) % len(pool)], :]
    return out


# ------------------------------------------------------------------------------------------ the transformer: one layer, then the forward
@functools.lru_cache(maxsize=None)
def sct_module(mode):
    c = sc.make_case(sc.SctCase("counted", C, F, 1, 1, 1, 8.0, 61))
    m = SelfCrossTransformer(d_model=C, nhead=sc.NHEAD, dim_feedforward=F, precision=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    m = m.to(DEV).eval()
    return m, m._pack(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def sct_inputs(B, N0, N1):
    rng = np.random.default_rng(1000 * B + N0 + N1)
    mk = lambda n, pos: torch.from_numpy((rng.uniform(-1, 1, (B, n, C)) if pos else rng.standard_normal((B, n, C))).astype(np.float32)).to(DEV)
    return mk(N0, False), mk(N0, True), mk(N1, False), mk(N1, True)


def exact_layer(mode, layer, x, px, mem=None, pm=None):
    """nl_sct_layer, the parent's exact-size entry."""
    _, packed = sct_module(mode)
    lib = _lib.load()
    x, px = x.contiguous(), px.contiguous()
    mem, pm = (x, px) if mem is None else (mem.contiguous(), pm.contiguous())
    B, Nq, Nk = x.shape[0], x.shape[1], mem.shape[1]
    out = torch.empty_like(x)
    need = lib.nl_sct_workspace_bytes(B, Nq, Nk, C, F)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_sct_layer(packed.data_ptr(), C, sc.NHEAD, F, layer, _lib.PRECISIONS[mode], x.data_ptr(), px.data_ptr(), Nq, mem.data_ptr(), pm.data_ptr(), Nk, B,
                                out.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "nl_sct_layer")
    return out


def counted_layer(mode, layer, x, px, mem, pm, nk):
    return _counted_lib.sct_layer_counted(sct_module(mode)[1], C, sc.NHEAD, F, layer, _lib.PRECISIONS[mode], x, px, mem, pm, nk)


def _layer_pair(mode, B, cap, n):
    """The self layer on the padded capacity and a cross layer with 40 queries on it, each counted, exact on n rows and un-counted on the padded rows."""
    v0, p0, v1, p1 = sct_inputs(B, cap, 40)
    xp, pp = _pad_rows(v0, n), _pad_rows(p0, n, 1.0)
    got = counted_layer(mode, 0, xp, pp, None, None, _cnt(n))
    want = exact_layer(mode, 0, v0[:, :n], p0[:, :n])
    plain = exact_layer(mode, 0, xp, pp)
    gotx = counted_layer(mode, 3, v1, p1, xp, pp, _cnt(n))
    wantx = exact_layer(mode, 3, v1, p1, v0[:, :n], p0[:, :n])
    plainx = exact_layer(mode, 3, v1, p1, xp, pp)
    return (got, want, plain), (gotx, wantx, plainx)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_counted_layer_has_the_bits_of_the_exact_size_layer(mode, n):
    (got, want, plain), (gotx, wantx, plainx) = _layer_pair(mode, 1, CAP, n)
    if n < CAP:   # the mask matters: the padded keys shift the un-counted result
        assert not _bits(plain[:, :n], want) and not _bits(plainx, wantx)
    else:
        assert _bits(plain, want) and _bits(plainx, wantx)
    assert tuple(got.shape) == (1, CAP, C) and _finite(got) and _bits(got[:, :n], want)
    assert _bits(gotx, wantx)


@pytest.mark.parametrize("mode", MODES)
def test_counted_layer_batch_stride_is_the_capacity(mode):
    (got, want, plain), (gotx, wantx, plainx) = _layer_pair(mode, 2, 130, 97)
    assert not _bits(plain[:, :97], want) and not _bits(plainx, wantx)
    assert _bits(got[:, :97], want) and _bits(gotx, wantx)
    assert tuple(got.shape) == (2, 130, C) and _finite(got)


@pytest.mark.parametrize("mode", MODES)
def test_counted_layer_count_zero_is_finite_and_clamps_hold(mode):
    v0, p0, v1, p1 = sct_inputs(1, 130, 40)
    xp, pp = _pad_rows(v0, 0), p0
    a, b = counted_layer(mode, 0, xp, pp, None, None, _cnt(0)), counted_layer(mode, 0, xp, pp, None, None, _cnt(0))
    ax, bx = counted_layer(mode, 3, v1, p1, xp, pp, _cnt(0)), counted_layer(mode, 3, v1, p1, xp, pp, _cnt(0))
    assert _finite(a) and _finite(ax) and _bits(a, b) and _bits(ax, bx)
    assert not _bits(a, exact_layer(mode, 0, xp, pp))
    # a negative count is zero, a count above the capacity is the capacity, and no count at all is nl_sct_layer
    assert _bits(counted_layer(mode, 0, xp, pp, None, None, _cnt(-5)), a) and _bits(counted_layer(mode, 3, v1, p1, xp, pp, _cnt(-1)), ax)
    full, fullx = exact_layer(mode, 0, xp, pp), exact_layer(mode, 3, v1, p1, xp, pp)
    assert _bits(counted_layer(mode, 0, xp, pp, None, None, _cnt(1000)), full) and _bits(counted_layer(mode, 3, v1, p1, xp, pp, _cnt(131)), fullx)
    assert _bits(counted_layer(mode, 0, xp, pp, None, None, None), full) and _bits(counted_layer(mode, 3, v1, p1, xp, pp, None), fullx)


@pytest.mark.parametrize("n", (1, 37, 97, 130))
@pytest.mark.parametrize("mode", MODES)
def test_counted_forward_has_the_bits_of_the_exact_size_forward(mode, n):
    m, packed = sct_module(mode)
    v0, p0, v1, p1 = sct_inputs(1, 130, 48)
    xp, pp = _pad_rows(v0, n), _pad_rows(p0, n, 1.0)
    want0, want1 = m.transform(v0[:, :n], p0[:, :n], v1, p1)         # nl_sct_forward
    plain0, plain1 = m.transform(xp, pp, v1, p1)
    if n < 130:
        assert not _bits(plain0[:, :n], want0) and not _bits(plain1, want1)
    got0, got1 = m.transform(xp, pp, v1, p1, n0=_cnt(n))
    assert tuple(got0.shape) == (1, 130, C) and _finite(got0) and _bits(got0[:, :n], want0) and _bits(got1, want1)
    if n == 130:   # no count at all: the bits of nl_sct_forward
        none0, none1 = _counted_lib.sct_forward_counted(packed, C, sc.NHEAD, F, _lib.PRECISIONS[mode], xp, pp, v1, p1, None)
        assert _bits(none0, want0) and _bits(none1, want1)
        zero0, zero1 = m.transform(xp, pp, v1, p1, n0=_cnt(0))
        assert _finite(zero0) and _finite(zero1)


# ------------------------------------------------------------------------------------------ the selection
def match_recipe(N, M, seed):
    """tests/match_cases.py's recipe at any (N, M): min(3 N / 4, M) rows get a planted partner."""
    rng = np.random.default_rng(seed)
    d0, d1 = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((M, C)).astype(np.float32)
    npl = min(max((3 * N) // 4, 1), M)
    perm = rng.permutation(M)[:npl]
    d1[perm] = d0[:npl] + np.float32(0.25) * rng.standard_normal((npl, C)).astype(np.float32)
    return d0, d1, npl


@functools.lru_cache(maxsize=None)
def s2d_module(mode):
    m = S2DMatching(C, thr=0.2, precision=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in mc.make_weights(C, 81).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("cap,M", [(1, 1), (65, 48), (130, 200), (1100, 70)])
@pytest.mark.parametrize("mode", MODES)
def test_counted_selection_equals_the_match_on_the_truncated_descriptors(mode, cap, M):
    m = s2d_module(mode)
    d0n, d1n, npl = match_recipe(cap, M, 7 * cap + M)
    d0, d1 = torch.from_numpy(d0n).to(DEV), torch.from_numpy(d1n).to(DEV)
    for n in sorted({0, 1, cap // 2, cap}):
        src = torch.arange(min(max(n, 1), npl), device=DEV)   # the valid rows with planted partners (n == 0: the first row)
        d0p = _pad_rows(d0, n, 8.0, src)
        _, plain_j, _ = m.match(d0p, d1)
        scores, got_j, got_s = m.match(d0p, d1, n=_cnt(n))
        assert got_j.dtype == torch.int32 and tuple(got_j.shape) == (cap,) and bool((got_j[n:] == -1).all()) and not bool(got_s[n:].any())
        ref_j, ref_s = cr.select_counted(scores.cpu().numpy(), n, 0.2)
        assert np.array_equal(got_j.cpu().numpy(), ref_j) and np.array_equal(got_s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))
        if n == 0:
            assert bool((plain_j >= 0).any())   # the padded rows do match when nothing masks them
            continue
        wscores, want_j, want_s = m.match(d0[:n].contiguous(), d1)   # nl_s2d_match
        assert _bits(scores[:n], wscores)   # a pair's score has its own bits whatever the other rows are
        if n < cap:
            assert not torch.equal(plain_j[:n], want_j), (n, "the padded rows take no match away")
        assert _bits(got_j[:n], want_j) and _bits(got_s[:n], want_s)
        print(f"{mode} ({cap}, {M}) n {n}: {int((want_j >= 0).sum())} matches, un-counted on the padded rows {int((plain_j[:n] >= 0).sum())}")


def test_counted_selection_on_planted_ties_equals_the_restatement():
    from tests import match_ref as mr
    N, M = 130, 200
    s = cr.tied_scores(N, M, 5)
    for n in (0, 1, 3, 65, 130, 200, -3):
        k = cr.clamp_count(n, N)
        sp = s.copy()
        sp[k:] = np.float32(0.99)   # would win every column
        got_j, got_s = _counted_lib.s2d_select_counted(torch.from_numpy(sp).to(DEV), _cnt(n), 0.2)
        ref_j, ref_s = cr.select_counted(sp, n, 0.2)
        assert np.array_equal(got_j.cpu().numpy(), ref_j) and np.array_equal(got_s.cpu().numpy(), ref_s)
        if k:
            assert np.array_equal(ref_j[:k], mr.select(s[:k], 0.2))
    none_j, _ = _counted_lib.s2d_select_counted(torch.from_numpy(s).to(DEV), None, 0.2)
    assert np.array_equal(none_j.cpu().numpy(), mr.select(s, 0.2)) and none_j[0] == 1 and none_j[1] == 2 and none_j[2] == 2


# ------------------------------------------------------------------------------------------ Matcher.forward_padded / localize with a count
PADDED_KEYS = ("i_ids", "j_ids", "b_ids", "mkps3d", "mkps2d_c", "expec_f", "mkps2d_f")
POSE_KEYS = ("T_w2c", "T_c2w", "num_inliers", "success", "best_candidate", "best_count")
IMAGE_K = (100.0, 100.0, 40.0, 30.0)
POSE_THR = 24.0
HYP, SEED = 256, 3


def geometric_kps3d(name, with_pixels=False):
    """tests/test_gpu_head.py's scene, restated: kps3d such that every planted pair satisfies one camera pose (with_pixels: and where each point projects)."""
    c = case(name)
    rng = np.random.default_rng(5)
    R, t = pc.rodrigues(0.3 * rng.normal(size=3)), np.array([0.1, -0.2, 0.3])
    N = c["case"].N
    px = rng.uniform(0, 60, size=(N, 2))
    ok = c["planted"] >= 0
    px[ok] = c["data"]["kps2d"][c["planted"][ok]] * hc.STRIDE_FINE
    depth = rng.uniform(2.0, 8.0, size=N)
    cam = np.stack([(px[:, 0] - IMAGE_K[2]) / IMAGE_K[0] * depth, (px[:, 1] - IMAGE_K[3]) / IMAGE_K[1] * depth, depth], axis=1)
    kps3d = ((cam - t) @ R).astype(np.float32)
    return (kps3d, px) if with_pixels else kps3d


@functools.lru_cache(maxsize=None)
def scene(name):
    m = build_matcher(name, precision="bf16x3").to(DEV).eval()
    data = tensors(case(name)["data"], DEV)
    data["kps3d"] = torch.from_numpy(geometric_kps3d(name)).to(DEV)
    return m, data


def exact_stage(m, data):
    """Matcher.forward and pose.absolute_pose: the parent's exact-size path."""
    with torch.no_grad():
        ref = m(dict(data))
    want = pose.absolute_pose(ref["mkps2d_f"] * data["stride_fine"], ref["mkps3d"], IMAGE_K, POSE_THR, hypotheses=HYP, seed=SEED)
    return ref, want


def _same_stage(got, ref, want, rows):
    M = len(ref["i_ids"])
    assert int(got["num_matches"]) == M and int(got["overflow"]) == 0
    for k in PADDED_KEYS:
        if M:
            assert _bits(got[k][:M], ref[k][:M]), k
        assert got[k].shape[0] == rows and _finite(got[k]), k
    for k in POSE_KEYS:
        assert _bits(got[k], want[k]), k
    assert tuple(got["inliers"].shape) == (rows,) and torch.equal(got["inliers"][:M], want["inliers"]) and not bool(got["inliers"][M:].any())


@pytest.mark.parametrize("name", hc.GOLDEN_CASES)
def test_localize_with_a_count_equals_forward_and_absolute_pose_on_the_first_rows(name):
    m, data = scene(name)
    N = case(name)["case"].N
    planted = torch.from_numpy(np.nonzero(case(name)["planted"] >= 0)[0]).to(DEV)
    for n in (3, N // 2, N):
        cut = dict(data)
        padded = dict(data)
        src = planted[planted < n]
        for k in cascade.POINT_KEYS:
            cut[k] = data[k][:n].contiguous()
            padded[k] = _pad_rows(data[k], n, 8.0 if k in ("desc_3d", "desc_3d_fine") else 1.0, src)
        ref, want = exact_stage(m, cut)
        plain = m.localize(padded, IMAGE_K, POSE_THR, hypotheses=HYP, seed=SEED)
        got = m.localize(padded, IMAGE_K, POSE_THR, hypotheses=HYP, seed=SEED, num_points=_cnt(n))
        M = len(ref["i_ids"])
        print(f"{name} n {n}: {M} matches, {int(want['num_inliers'])} inliers, success {int(want['success'])}; un-counted on the padded rows: {int(plain['num_matches'])} matches")
        if n < N:
            assert int(plain["num_matches"]) != M or not _bits(plain["i_ids"][:M], ref["i_ids"])   # the mask matters
        else:   # with every row counted the results carry the bits of the call without a count
            for k in PADDED_KEYS + POSE_KEYS + ("inliers", "num_matches", "score_matrix"):
                assert _bits(got[k], plain[k]), k
        _same_stage(got, ref, want, N)
        fp = m.forward_padded(padded, num_points=_cnt(n))
        assert int(fp["num_matches"]) == M and all(_bits(fp[k][:M], ref[k][:M]) for k in PADDED_KEYS if M)
        assert _bits(fp["score_matrix"][:n], ref["score_matrix"])
    assert int(want["success"]) == 1 and int(want["num_inliers"]) >= 8   # n == N: the scene's pose is found


def test_localize_with_a_count_of_zero_gives_the_identity():
    m, data = scene("head64")
    got = m.localize(data, IMAGE_K, POSE_THR, hypotheses=64, num_points=_cnt(0))
    assert int(got["num_matches"]) == 0 and int(got["success"]) == 0 and int(got["num_inliers"]) == 0 and not bool(got["inliers"].any())
    eye = torch.eye(4, dtype=torch.float64, device=DEV)
    assert torch.equal(got["T_w2c"], eye) and torch.equal(got["T_c2w"], eye)
    assert all(_finite(got[k]) for k in PADDED_KEYS + ("score_matrix", "pts2d"))


# ------------------------------------------------------------------------------------------ the cascade
CASCADE_KEYS = ("T_c2w", "T_w2c", "num_points", "stage")
STAGE2_KEYS = POSE_KEYS + ("inliers", "num_matches", "overflow")


@functools.lru_cache(maxsize=None)
def cascade_scene():
    m, data = scene("head64")
    mf = build_matcher("head64", precision="bf16x3").to(DEV).eval()
    mf.coarse_matcher.thr = 0.25   # a second matcher of its own: not the first one's selection
    return m, mf, data


def exact_cascade(m, mf, data, H, W):
    """The parent's way: localize, select_3d_keypoints (one read-back), indexing, forward (two read-backs), absolute_pose."""
    s1 = m.localize(data, IMAGE_K, POSE_THR, hypotheses=HYP, seed=SEED)
    Kd = torch.tensor([[IMAGE_K[0], 0, IMAGE_K[2]], [0, IMAGE_K[1], IMAGE_K[3]], [0, 0, 1]], dtype=torch.float32, device=DEV)
    idx = keypoints.select_3d_keypoints(data["kps3d"], s1["T_c2w"][None], Kd, H, W)
    n = len(idx)
    if n == 0:
        return {"T_c2w": s1["T_c2w"], "T_w2c": s1["T_w2c"], "n": 0, "stage": 1, "idx": idx, "stage1": s1}
    sub = dict(data)
    for k in cascade.POINT_KEYS:
        sub[k] = data[k][idx]
    ref, want = exact_stage(mf, sub)
    return {"T_c2w": want["T_c2w"], "T_w2c": want["T_w2c"], "n": n, "stage": 2, "idx": idx, "stage1": s1, "ref": ref, "want": want}


def test_cascade_equals_the_composition_of_the_exact_size_forms():
    m, mf, data = cascade_scene()
    N = case("head64")["case"].N
    ex = exact_cascade(m, mf, data, 60, 30)
    print(f"cascade head64 (H, W) = (60, 30): stage two sees {ex['n']} of {N} points, {len(ex['ref']['i_ids'])} matches")
    assert 4 < ex["n"] < N
    got = cascade.localize_cascade(m, mf, data, IMAGE_K, 60, 30, POSE_THR, hypotheses=HYP, seed=SEED)
    assert all(got[k].is_cuda for k in CASCADE_KEYS) and got["T_c2w"].dtype == torch.float64 and got["num_points"].dtype == torch.int32
    assert int(got["num_points"]) == ex["n"] and int(got["stage"]) == 2 and torch.equal(got["idx"][:ex["n"]], ex["idx"]) and not bool(got["idx"][ex["n"]:].any())
    assert _bits(got["T_c2w"], ex["T_c2w"]) and _bits(got["T_w2c"], ex["T_w2c"])
    _same_stage(got["stage2"], ex["ref"], ex["want"], N)
    for k in POSE_KEYS + ("inliers", "num_matches"):
        assert _bits(got["stage1"][k], ex["stage1"][k]), k
    assert not _bits(got["T_c2w"], got["stage1"]["T_c2w"])
    # bounds that see no point: stage one's pose.  The window starts at the image origin, where the scene has a planted cell; the points that project within
    # 5 pixels of the 1 x 1 window (the estimated pose is exact to a pixel or two) become copies of the point farthest from it, so the next one is 7 pixels away
    kps3d, px = geometric_kps3d("head64", with_pixels=True)
    dist = np.maximum(np.abs(px - 0.5) - 0.5, 0).max(axis=1)
    kps3d[dist < 5.0] = kps3d[dist.argmax()]
    assert 0 < (dist < 5.0).sum() <= 3 and np.sort(dist)[(dist < 5.0).sum()] >= 7.0
    data = {**data, "kps3d": torch.from_numpy(kps3d).to(DEV)}
    none = exact_cascade(m, mf, data, 1, 1)
    print(f"cascade head64 (H, W) = (1, 1): stage two sees {none['n']} points")
    assert none["n"] == 0
    got = cascade.localize_cascade(m, mf, data, IMAGE_K, 1, 1, POSE_THR, hypotheses=HYP, seed=SEED)
    assert int(got["num_points"]) == 0 and int(got["stage"]) == 1 and _bits(got["T_c2w"], none["T_c2w"]) and _bits(got["T_w2c"], none["T_w2c"])
    assert int(got["stage2"]["success"]) == 0 and torch.equal(got["stage2"]["T_c2w"], torch.eye(4, dtype=torch.float64, device=DEV))
    assert all(_finite(got["stage2"][k]) for k in PADDED_KEYS)


def test_cascade_replays_from_a_captured_graph():
    """One capture after a warm call; two replays with other descriptors copied into the static inputs; each equals the eager call's bits.  A host synchronisation
    or an allocation outside torch's allocator during the capture would be an error, so the captured call made none.

    Both stages are compared, key by key.  (While stage one took nl_s2d_match's own selection, whose maxima a memset node clears, this test failed in 7 of 9
    runs of this file — stage one's replay lost matches, its scores being right — and in none of 6 with a kernel clearing them: DESIGN 5.45.)"""
    m, mf, data = cascade_scene()
    run = lambda d: cascade.localize_cascade(m, mf, d, IMAGE_K, 60, 30, POSE_THR, hypotheses=HYP, seed=SEED)

    def snapshot(r):
        k2 = int(r["stage2"]["num_matches"])
        out = {k: r[k].clone() for k in CASCADE_KEYS}
        out.update({"1." + k: r["stage1"][k].clone() for k in STAGE2_KEYS})
        out.update({"2." + k: r["stage2"][k].clone() for k in STAGE2_KEYS})
        out.update({"2." + k: r["stage2"][k][:k2].clone() for k in PADDED_KEYS})
        return out
    variants = []
    for shift in (1, 0):   # the coarse map's descriptors rolled by a cell (every partner, and with it stage one's pose, moves 8 pixels: another count), then the recipe's own
        d2 = torch.roll(data["desc_2d_coarse"], shift, 0).clone()
        variants.append((d2, snapshot(run({**data, "desc_2d_coarse": d2}))))
    counts = [int(v["num_points"]) for _, v in variants]
    print("stage-two counts of the two replays:", counts)
    assert counts[0] != counts[1]
    static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}
    run(static)   # the warm call: weight images, the cached intrinsics
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run(static)
    for d2, eager in variants:
        for k in CASCADE_KEYS:
            cap[k].zero_()
        static["desc_2d_coarse"].copy_(d2)
        g.replay()
        torch.cuda.synchronize()
        now = snapshot(cap)
        bad = [k for k, v in eager.items() if not _bits(now[k], v)]
        assert not bad, " ".join(bad)
