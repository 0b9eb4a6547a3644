"""Recipes of the keypoint-geometry tests (tests/test_geom_cpu.py, tests/test_gpu_geom.py) and of tools/gen_geom_golden.py.

Inputs are regenerated from the seeds below, never stored; tests/golden/geom_*.npz hold what the reference's select_3d_keypoints / build_3d_2d_pairs make of them.
Only rng.random() and IEEE arithmetic are used (rotations by the Cayley transform, no sine), so a recipe is the same on every machine.

GUARD BAND.  The decisions (valid, depth_ok, the pixel and the cell a point falls into) are discontinuous; the reference takes them in fp32, the library in fp64,
and the tests demand the reference's decisions on EVERY point.  So points are rejection-sampled, in fp64 (tests/geom_ref.py), until for every pose of the recipe
  |u|, |u - W|, |v|, |v - H| >= BAND_PX;   |z| >= BAND_Z
and, for the query pose and the points valid in it, additionally
  u and v are at least BAND_PX away from the next integer (the pixel of the depth read; a multiple of the stride is an integer, so the cell too)
  | |depth - z| - thr | >= BAND_DEPTH.
The reference's formulas in fp32 against fp64, over 200 random poses x 4096 points at 640 x 480, f = 525, z >= 0.05, differ by at most 1.1e-3 px in u, v and
2.1e-6 in z; the band is about 18 times that, and the generator re-measures the deviation per recipe and refuses a recipe whose band is not 8 times its own.
The `edge` recipe has no band: its coordinates are exact in fp32 and fp64 alike and sit ON the borders.
"""
import os
from collections import namedtuple

import numpy as np

from tests import geom_ref as gr

BAND_PX, BAND_Z, BAND_DEPTH = 0.02, 1e-3, 1e-4

Case = namedtuple("Case", "name N V H W stride f thr kind seed")
CASES = {c.name: c for c in (
    Case("small", 200, 3, 48, 64, 8, 60.0, 0.05, "scene", 31),
    Case("views10", 2048, 10, 480, 640, 8, 525.0, 0.05, "scene", 32),        # points behind the cameras and outside every view among them
    Case("none_visible", 300, 3, 48, 64, 8, 60.0, 0.05, "behind", 33),       # every point behind every camera
    Case("fallback", 300, 2, 48, 64, 8, 60.0, 0.05, "fallback", 34),         # at most 3 depth-consistent points: the positive set is `valid`
    Case("no_valid", 130, 1, 48, 64, 4, 60.0, 0.05, "behind", 35),           # nothing projects into the query view: no pair at all
    Case("depth_points", 500, 2, 96, 128, 8, 120.0, 0.05, "points", 36),     # the per-point depth source
    Case("nonrigid", 400, 3, 48, 64, 8, 60.0, 0.05, "nonrigid", 37),         # a 1e-3 shear in every pose: the general inverse, not the transpose
    Case("edge", 0, 1, 48, 64, 8, 256.0, 0.5, "edge", 38),                   # N follows from the construction
)}
GOLDEN_CASES = tuple(CASES)


def intrinsics(c):
    return np.array([[c.f, 0.0, c.W / 2.0], [0.0, c.f, c.H / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)


def cayley(s):
    """The rotation (I - S)^-1 (I + S) of the skew matrix S of s: arithmetic only."""
    S = np.array([[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]])
    return np.linalg.solve(np.eye(3) - S, np.eye(3) + S)


def make_pose(rng, shear=0.0, spread=0.3):
    """A c2w pose near the origin looking along +z, rounded to fp32 (so it is never exactly rigid)."""
    T = np.eye(4)
    T[:3, :3] = cayley(spread * (2.0 * rng.random(3) - 1.0))
    if shear:
        T[:3, :3] = T[:3, :3] @ np.array([[1.0, shear, 0.0], [0.0, 1.0, shear], [shear, 0.0, 1.0]])
    T[:3, 3] = 0.5 * (2.0 * rng.random(3) - 1.0)
    return T.astype(np.float32)


def sample_points(rng, n, kind):
    p = rng.random((n, 3))
    if kind == "behind":
        return (p * [6.0, 6.0, 5.0] + [-3.0, -3.0, -7.0]).astype(np.float32)
    return (p * [8.0, 8.0, 9.0] + [-4.0, -4.0, -3.0]).astype(np.float32)


def band_violations(pts, poses, query, K, H, W):
    """bool (N): the points that sit inside the band of a geometric decision."""
    bad = np.zeros(len(pts), dtype=bool)
    for n, pose in enumerate(list(poses) + [query]):
        u, v, z, valid = gr.project(pts, pose, K, H, W)
        with np.errstate(all="ignore"):
            near = (np.abs(u) < BAND_PX) | (np.abs(u - W) < BAND_PX) | (np.abs(v) < BAND_PX) | (np.abs(v - H) < BAND_PX) | (np.abs(z) < BAND_Z)
            near |= ~(np.isfinite(u) & np.isfinite(v))
            if n == len(poses):
                near |= valid & ((np.abs(u - np.rint(u)) < BAND_PX) | (np.abs(v - np.rint(v)) < BAND_PX))
        bad |= near
    return bad


def depth_violations(pts, query, K, H, W, thr, depth, depth_points):
    u, v, z, valid = gr.project(pts, query, K, H, W)
    vi = np.nonzero(valid)[0]
    d = depth[vi].astype(np.float64) if depth_points else depth[np.trunc(v[vi]).astype(int), np.trunc(u[vi]).astype(int)].astype(np.float64)
    bad = np.zeros(len(pts), dtype=bool)
    bad[vi] = np.abs(np.abs(d - z[vi]) - thr) < BAND_DEPTH
    return bad


def make_depth(rng, c, pts, query, K, consistent_share, max_consistent=None):
    """The depth source of the query view: z of a share of the valid points (the others are off by 0.3 .. 1.3), 0 where no point falls."""
    u, v, z, valid = gr.project(pts, query, K, c.H, c.W)
    off = np.where(rng.random(len(pts)) < consistent_share, 0.0, 0.3 + rng.random(len(pts)))
    if max_consistent is not None:
        keep = np.nonzero(valid & (off == 0.0))[0][max_consistent:]
        off[keep] = 0.7
    if c.kind == "points":
        return np.where(np.isfinite(z), z + off, 0.0).astype(np.float32)
    depth = np.zeros((c.H, c.W), dtype=np.float32)
    vi = np.nonzero(valid)[0]
    depth[np.trunc(v[vi]).astype(int), np.trunc(u[vi]).astype(int)] = (z[vi] + off[vi]).astype(np.float32)   # two points in a pixel: the later one wins
    return depth


def make_edge_case(c):
    """Identity pose, f = 256 (a power of two), z in {1, 2, 4} and x, y = z (target - centre) / 256: u, v are the integer targets exactly, in fp32 and in fp64 —
    on the image borders (0, W, H: >= against <), one pixel to either side, and on the cell borders.  Also z = 0 (u = NaN or inf) and z < 0."""
    K = intrinsics(c)
    us = [-1, 0, 1, 7, 8, 9, 16, c.W - 1, c.W, c.W + 1]
    vs = [-1, 0, 1, 8, 15, 16, c.H - 1, c.H, c.H + 1]
    rows = [((ut - c.W / 2.0) * z / c.f, (vt - c.H / 2.0) * z / c.f, z) for n, (ut, vt) in enumerate((a, b) for a in us for b in vs) for z in (float(1 << (n % 3)),)]
    rows += [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), (0.25, 0.25, -2.0)]
    pts = np.array(rows, dtype=np.float32)
    assert np.array_equal(pts.astype(np.float64), np.array(rows))   # exact in fp32
    pose = np.eye(4, dtype=np.float32)
    depth = np.zeros((c.H, c.W), dtype=np.float32)
    for n, (ut, vt) in enumerate((a, b) for a in us for b in vs):
        if 0 <= ut < c.W and 0 <= vt < c.H:
            depth[vt, ut] = float(1 << (n % 3)) + (0.0 if n % 2 else 1.0)   # every other point consistent; |depth - z| is 0 or 1 against thr = 0.5
    return {"case": c._replace(N=len(pts)), "pts": pts, "poses": pose[None].copy(), "query": pose, "K": K, "depth": depth, "depth_points": False}


def make_case(name):
    """-> dict(case, pts (N, 3), poses (V, 4, 4), query (4, 4), K (3, 3), depth (H, W) or (N), depth_points), all fp32."""
    c = CASES[name]
    if c.kind == "edge":
        return make_edge_case(c)
    rng = np.random.default_rng(c.seed)
    K = intrinsics(c)
    shear = 1e-3 if c.kind == "nonrigid" else 0.0
    poses = np.stack([make_pose(rng, shear) for _ in range(c.V)])
    query = make_pose(rng, shear, spread=0.1)
    pts = sample_points(rng, c.N, c.kind)
    todo = np.ones(c.N, dtype=bool)
    for _ in range(200):
        while True:
            bad = band_violations(pts, poses, query, K, c.H, c.W) & todo   # only re-drawn points can be new offenders
            if not bad.any():
                break
            pts[bad] = sample_points(rng, int(bad.sum()), c.kind)
            todo = bad
        depth = make_depth(rng, c, pts, query, K, 0.6, 3 if c.kind == "fallback" else None)
        bad = depth_violations(pts, query, K, c.H, c.W, c.thr, depth, c.kind == "points")
        if not bad.any():
            break
        pts[bad] = sample_points(rng, int(bad.sum()), c.kind)
        todo = bad
    else:
        raise AssertionError(f"{name}: no sample outside the guard band")
    return {"case": c, "pts": pts, "poses": poses, "query": query, "K": K, "depth": depth, "depth_points": c.kind == "points"}


def excluded_share(case):
    """The share of points a comparison would have to leave out: those inside the band.  0 for every recipe by construction (`edge`: no band, nothing left out)."""
    c = case["case"]
    if c.kind == "edge":
        return 0.0
    bad = band_violations(case["pts"], case["poses"], case["query"], case["K"], c.H, c.W)
    bad |= depth_violations(case["pts"], case["query"], case["K"], c.H, c.W, c.thr, case["depth"], case["depth_points"])
    return float(bad.mean())


def sweep_inputs(N, V, seed, H=48, W=64, f=60.0, kind="scene"):
    """pts (N, 3), poses (V, 4, 4), query, K for the shape sweeps held to the restatement, outside the geometric band of every pose."""
    rng = np.random.default_rng(seed)
    c = Case("sweep", N, V, H, W, 8, f, 0.05, kind, seed)
    K = intrinsics(c)
    poses = np.stack([make_pose(rng) for _ in range(V)])
    query = make_pose(rng, spread=0.1)
    pts = sample_points(rng, N, kind)
    for _ in range(200):
        bad = band_violations(pts, poses, query, K, H, W)
        if not bad.any():
            return pts, poses, query, K
        pts[bad] = sample_points(rng, int(bad.sum()), kind)
    raise AssertionError("sweep_inputs: no sample outside the guard band")


def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(golden_dir(), f"geom_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def expected(case, g):
    """What a golden file pins, in the library's terms: mask / valid from the reference's index lists, gt_j from its pairs (-1 off the positive set)."""
    N = case["case"].N
    mask, valid = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    mask[g["vis_idx"]] = True
    valid[g["valid_idx"]] = True
    gt_j = np.full(N, -1, dtype=np.int32)
    gt_j[g["pairs"][0]] = g["pairs"][1]
    return {"mask": mask, "vis_idx": g["vis_idx"].astype(np.int64), "valid": valid, "pairs": g["pairs"].astype(np.int64), "gt_j": gt_j,
            "used_fallback": int(g["used_fallback"]), "proj64": g["proj64"]}


def proj_error(proj, ref64, rows=None):
    """max |err| / max |ref| over the rows whose reference is finite (`rows`: a further restriction, e.g. the valid points); 0 if there is no such row."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    keep = np.isfinite(ref64).all(axis=1) if rows is None else np.isfinite(ref64).all(axis=1) & rows
    if not keep.any():
        return 0.0
    return float(np.abs(np.asarray(proj, dtype=np.float64)[keep] - ref64[keep]).max() / max(np.abs(ref64[keep]).max(), 1e-300))


def sweep_depth(pts, query, K, H, W, thr, seed, points):
    """A depth source for sweep_inputs' points — per point (z, or z + 0.5 for every other point) or the map make_depth builds — outside the depth band."""
    c = Case("sweep", len(pts), 1, H, W, 8, 0.0, thr, "points" if points else "scene", seed)
    if points:
        z = gr.project(pts, query, K, H, W)[2]
        depth = np.where(np.isfinite(z), z + 0.5 * (np.arange(len(pts)) % 2), 0.0).astype(np.float32)
    else:
        depth = make_depth(np.random.default_rng(seed), c, pts, query, K, 0.6)
    assert not depth_violations(pts, query, K, H, W, thr, depth, points).any(), "sweep_depth: choose another seed"
    return depth
