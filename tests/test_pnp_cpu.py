"""CPU-side tests of the absolute-pose solver (csrc/pnp.hip as restated in tests/pnp_ref.py): the sampler, the restatement against the ground truth of the
synthetic scenes, the six new symbols, the argument checks that need no GPU and the workspace query."""
import ctypes as ct
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import pnp_cases as pc
from tests import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNP_SYMBOLS = ("nl_pnp_workspace_bytes", "nl_pnp_samples", "nl_pnp_hypotheses", "nl_pnp_score", "nl_pnp_refine", "nl_pnp_ransac")


@functools.lru_cache(maxsize=None)
def solved(name):
    s = pc.make_case(name)
    c = s["case"]
    return s, pr.ransac(s["pts2d"], s["pts3d"], pc.K, c.thr, c.H, seed=0)


@pytest.mark.parametrize("M", (3, 4, 5, 65, 1024, 1 << 20))
def test_samples_are_distinct_and_in_range(M):
    for b in (0, 2):
        idx = pr.samples(0x1234567890ABCDEF, b, 256, M).astype(np.int64)
        assert idx.shape == (256, 3) and idx.min() >= 0 and idx.max() < M
        assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 0] != idx[:, 2]).all() and (idx[:, 1] != idx[:, 2]).all()
    assert (pr.samples(0, 0, 64, 2) == -1).all()


def test_samples_are_a_function_of_seed_problem_and_sample_alone():
    a = pr.samples(7, 1, 256, 100)
    assert np.array_equal(pr.samples(7, 1, 64, 100), a[:64])                     # H does not enter
    assert not np.array_equal(pr.samples(8, 1, 256, 100), a) and not np.array_equal(pr.samples(7, 2, 256, 100), a)
    assert not np.array_equal(pr.samples(7 + (1 << 32), 1, 256, 100), a)         # the seed's high word is part of the key
    assert set(pr.samples(0, 0, 64, 4).reshape(-1).tolist()) == {0, 1, 2, 3}   # with M = 4 every index is hit: the sampler covers the range


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_restatement_recovers_the_ground_truth(name):
    s, r = solved(name)
    c = s["case"]
    n_true = int((~s["is_outlier"]).sum())
    assert r["success"] == 1 and r["best_count"] == r["counts"].max() and r["best_candidate"] == int(np.nonzero(r["counts"] == r["counts"].max())[0][0])
    ang, dist = pc.pose_error(r["pose"], s["R"], s["t"])
    assert ang <= pc.GT_BARS[name][0] and dist <= pc.GT_BARS[name][1], (ang, dist)
    # the mask is the true-inlier labels except for outliers that truly reproject inside thr
    gt = np.concatenate([s["R"], s["t"][:, None]], axis=1).reshape(12)
    lucky = s["is_outlier"] & pr.inlier_mask(gt, s["pts2d"], s["pts3d"], pc.K, c.thr)
    assert np.array_equal(r["mask"], ~s["is_outlier"] | lucky) and r["num_inliers"] == n_true + int(lucky.sum()) and lucky.sum() <= 2
    # ties are the normal case: the best candidates all hold the same count
    assert (np.sort(r["counts"])[-4:] == r["best_count"]).all()


@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_restated_p3p_solutions_reproduce_their_pixels(name):
    s, r = solved(name)
    idx = r["samples"].astype(np.int64)
    worst = []
    for h in range(s["case"].H):
        for k in range(r["nsol"][h]):
            e2, z = pr.reproject(r["poses"][h, k], s["pts2d"][idx[h]], s["pts3d"][idx[h]], pc.K)
            assert (z > 0).all()
            worst.append(np.sqrt(e2.max()))
    worst = np.array(worst)
    assert worst.size >= s["case"].H and worst.max() <= 1e-3 and (worst > 1e-6).mean() <= 0.01
    if name in pc.NOISE_FREE:   # one solution of every sample is the ground truth
        for h in range(s["case"].H):
            errs = [pc.pose_error(r["poses"][h, k], s["R"], s["t"]) for k in range(r["nsol"][h])]
            assert errs and min(e[0] for e in errs) <= 1e-2 and min(e[1] for e in errs) <= 1e-3, h


def test_degenerate_and_short_problems():
    s = pc.make_case("clean65")
    same2, same3 = np.repeat(s["pts2d"][:1], 8, axis=0), np.repeat(s["pts3d"][:1], 8, axis=0)
    r = pr.ransac(same2, same3, pc.K, 8.0, 64)
    assert (r["nsol"] == 0).all() and (r["counts"] == -1).all() and r["success"] == 0 and np.array_equal(r["pose"], pr.IDENTITY) and not r["mask"].any()
    for M in (0, 3):
        r = pr.ransac(s["pts2d"][:M], s["pts3d"][:M], pc.K, 8.0, 64)
        assert r["success"] == 0 and r["num_inliers"] == 0 and np.array_equal(r["pose"], pr.IDENTITY) and r["mask"].shape == (M,) and not r["mask"].any()
    # collinear world points: a triangle of zero area
    line = np.stack([np.linspace(0, 1, 8), np.zeros(8), np.full(8, 5.0)], axis=1).astype(np.float32)
    assert (pr.hypotheses(s["pts2d"][:8], line, pc.K, 0, 0, 64)[2] == 0).all()


def _declared():
    src = open(os.path.join(ROOT, "include", "nerfloc_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nl_[a-z_0-9]+)\s*\(", src)))


def test_header_binding_and_library_agree_on_104_symbols():
    declared = _declared()
    assert len(declared) == 104 and set(PNP_SYMBOLS) <= set(declared)
    assert sorted(n for n, _, _ in _lib.SYMBOLS) == declared
    res = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    assert sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip()) == declared
    hdr = open(os.path.join(ROOT, "include", "nerfloc_render.h")).read()
    assert int(re.search(r"#define\s+NL_PNP_LO_ROUNDS\s+(\d+)", hdr).group(1)) == pr.LO_ROUNDS
    assert int(re.search(r"#define\s+NL_PNP_GN_ITERS\s+(\d+)", hdr).group(1)) == pr.GN_ITERS
    assert _lib.load().nl_abi_version() == 13 and _lib.ABI_VERSION == 13


def test_workspace_query_is_monotone_and_linear_in_the_problems():
    lib = _lib.load()
    w = lib.nl_pnp_workspace_bytes
    one = w(1024, 1, 1024)
    assert one > 0 and one % 256 == 0
    for B in (2, 3, 8, 17):
        assert w(1024 * B, B, 1024) == B * one
    assert w(0, 0, 64) == 0
    for H in (64, 128, 1024, 65536):
        assert w(100, 2, H) <= w(100, 2, H + 64 if H < 65536 else H) and w(100, 2, H) <= w(100, 3, H) and w(100, 2, H) <= w(200, 2, H)
    assert w(100, 1, 64) < w(100, 1, 128) < w(100, 1, 65536)
    assert w(-1, 1, 64) == 0 and w(10, -1, 64) == 0 and w(10, 1, 0) == 0 and w(10, 1, 96) == 0 and w(10, 1, 65536 + 64) == 0


def test_arguments_are_validated_before_anything_is_dereferenced():
    """No GPU needed: the device pointers are host buffers (or null) that a correct library never reads; every call below must be refused, or has nothing to do."""
    lib = _lib.load()
    OK, BAD, UNS, WS = _lib.NL_OK, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    buf = (ct.c_char * 8192)()
    p = ct.c_void_p((ct.addressof(buf) + 255) // 256 * 256)
    q = ct.c_void_p(p.value + 4)
    i32, f64 = lambda *v: (ct.c_int32 * len(v))(*v), lambda *v: (ct.c_double * len(v))(*v)
    off2, K2, thr2 = i32(0, 5, 12), f64(500, 500, 320, 240, 400, 410, 300, 200), f64(8, 2)
    need = lib.nl_pnp_workspace_bytes(12, 2, 64)
    nan, inf = float("nan"), float("inf")

    def ransac(p2=p, p3=p, off=off2, K=K2, thr=thr2, B=2, H=64, seed=1, min_inliers=4, poses=p, mask=p, info=p, counts=None, ws=p, ws_bytes=None):
        return lib.nl_pnp_ransac(p2, p3, off, K, thr, B, H, seed, min_inliers, poses, mask, info, counts, ws, need - 1 if ws_bytes is None else ws_bytes, None)
    # every call has a short workspace unless it says otherwise: nothing may be launched
    assert ransac() == WS and ransac(ws=None, ws_bytes=need) == WS and ransac(ws=q, ws_bytes=need) == WS and ransac(ws_bytes=0) == WS
    assert ransac(p2=None) == BAD and ransac(p3=None) == BAD and ransac(poses=None) == BAD and ransac(mask=None) == BAD and ransac(info=None) == BAD
    assert ransac(off=None) == BAD and ransac(K=None) == BAD and ransac(thr=None) == BAD and ransac(B=-1) == BAD
    assert ransac(off=i32(0, 7, 5)) == BAD and ransac(off=i32(1, 5, 12)) == BAD and ransac(off=i32(0, -1, 12)) == BAD
    for bad in (0.0, -8.0, nan, inf):
        assert ransac(thr=f64(8, bad)) == BAD and ransac(K=f64(500, 500, 320, 240, bad, 410, 300, 200)) == BAD
        assert ransac(K=f64(500, bad, 320, 240, 400, 410, 300, 200)) == BAD
    assert ransac(K=f64(500, 500, nan, 240, 400, 410, 300, 200)) == BAD and ransac(K=f64(500, 500, 320, 240, 400, 410, 300, inf)) == BAD
    assert ransac(min_inliers=3) == BAD and ransac(min_inliers=0) == BAD and ransac(min_inliers=-4) == BAD
    for H in (0, 32, 63, 96, 65536 + 64, -64):
        assert ransac(H=H) == UNS
    assert ransac(off=i32(0, 5, 5 + (1 << 20) + 1)) == UNS
    assert ransac(B=0, p2=None, p3=None, off=None, K=None, thr=None, poses=None, mask=None, info=None, ws=None, ws_bytes=0) == OK
    # empty problems need no match pointers; the workspace is still checked
    assert ransac(off=i32(0, 0, 0), p2=None, p3=None, mask=None) == WS

    def samples(seed=1, off=off2, B=2, H=64, out=p):
        return lib.nl_pnp_samples(seed, off, B, H, out, None)
    assert samples(out=None) == BAD and samples(off=None) == BAD and samples(off=i32(0, 7, 5)) == BAD and samples(B=-1) == BAD and samples(H=100) == UNS
    assert samples(off=i32(0, 5, 5 + (1 << 20) + 1)) == UNS and samples(B=0, off=None, out=None) == OK

    def hyp(p2=p, p3=p, off=off2, K=K2, B=2, H=64, seed=1, smp=None, poses=p, nsol=p):
        return lib.nl_pnp_hypotheses(p2, p3, off, K, B, H, seed, smp, poses, nsol, None)
    assert hyp(p2=None) == BAD and hyp(p3=None) == BAD and hyp(poses=None) == BAD and hyp(nsol=None) == BAD and hyp(off=None) == BAD and hyp(K=None) == BAD
    assert hyp(off=i32(0, 7, 5)) == BAD and hyp(K=f64(500, 0, 320, 240, 400, 410, 300, 200)) == BAD and hyp(B=-1) == BAD and hyp(H=65) == UNS
    assert hyp(off=i32(0, 5, 5 + (1 << 20) + 1)) == UNS and hyp(B=0, p2=None, p3=None, off=None, K=None, poses=None, nsol=None) == OK

    K1 = f64(500, 500, 320, 240)

    def score(p2=p, p3=p, M=5, K=K1, thr=8.0, poses=p, nsol=None, P=8, counts=p):
        return lib.nl_pnp_score(p2, p3, M, K, thr, poses, nsol, P, counts, None)
    assert score(p2=None) == BAD and score(p3=None) == BAD and score(poses=None) == BAD and score(counts=None) == BAD and score(K=None) == BAD
    assert score(M=-1) == BAD and score(P=-1) == BAD and score(nsol=p, P=6) == BAD and score(K=f64(-1, 500, 320, 240)) == BAD
    for bad in (0.0, -1.0, nan, inf):
        assert score(thr=bad) == BAD
    assert score(M=(1 << 20) + 1) == UNS and score(P=0, poses=None, counts=None) == OK

    def refine(p2=p, p3=p, M=5, K=K1, thr=8.0, min_inliers=4, pin=p, pout=p, mask=p, info=p):
        return lib.nl_pnp_refine(p2, p3, M, K, thr, min_inliers, pin, pout, mask, info, None)
    assert refine(p2=None) == BAD and refine(p3=None) == BAD and refine(pin=None) == BAD and refine(pout=None) == BAD and refine(mask=None) == BAD
    assert refine(info=None) == BAD and refine(K=None) == BAD and refine(M=-1) == BAD and refine(min_inliers=3) == BAD and refine(thr=nan) == BAD
    assert refine(K=f64(500, inf, 320, 240)) == BAD and refine(M=(1 << 20) + 1) == UNS


def test_module_refuses_cpu_tensors_and_bad_arguments():
    from nerf_loc_amd import pose
    s = pc.make_case("min4")
    p2, p3 = torch.from_numpy(s["pts2d"]), torch.from_numpy(s["pts3d"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.absolute_pose(p2, p3, pc.K, 8.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.estimate_pose(p2, p3, torch.eye(3), 640, 480)
    assert pose.absolute_pose_batch([]) == []
    assert pose._intrinsics(torch.tensor([[500.0, 0, 320], [0, 510, 240], [0, 0, 1]])) == (500.0, 510.0, 320.0, 240.0)
    assert pose._intrinsics(np.array([[500.0, 0, 320], [0, 510, 240], [0, 0, 1]])) == (500.0, 510.0, 320.0, 240.0)
    assert pose._intrinsics((1, 2, 3, 4)) == (1.0, 2.0, 3.0, 4.0)
    with pytest.raises(ValueError):
        pose._intrinsics((1, 2, 3))
