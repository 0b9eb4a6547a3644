"""The contracts of include/nerfloc_geom.h restated in numpy, fp64 throughout, one rounding per written operation and sums left to right as the header writes them
(numpy's element-wise operations fuse nothing).  Written from the header's text; the tests hold the library, the eager CPU path and the goldens to it."""
import numpy as np

MIN_POSITIVES = 4


def combined_matrix(pose, K):
    """P (3, 4) = K [R | t], [R | t] the inverse of the affine map in the top three rows of the 4 x 4 c2w `pose`: adjugate / determinant."""
    A = np.asarray(pose, dtype=np.float64)[:3, :3]
    c = np.asarray(pose, dtype=np.float64)[:3, 3]
    k = np.asarray(K, dtype=np.float64)
    C = np.empty((3, 3))
    C[0, 0] = A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]
    C[0, 1] = A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2]
    C[0, 2] = A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]
    C[1, 0] = A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2]
    C[1, 1] = A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0]
    C[1, 2] = A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1]
    C[2, 0] = A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]
    C[2, 1] = A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]
    C[2, 2] = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    det = A[0, 0] * C[0, 0] + A[0, 1] * C[0, 1] + A[0, 2] * C[0, 2]
    with np.errstate(all="ignore"):
        R = C.T / det
    t = np.array([-(R[r, 0] * c[0] + R[r, 1] * c[1] + R[r, 2] * c[2]) for r in range(3)])
    P = np.empty((3, 4))
    for r in range(3):
        for q in range(3):
            P[r, q] = k[r, 0] * R[0, q] + k[r, 1] * R[1, q] + k[r, 2] * R[2, q]
        P[r, 3] = k[r, 0] * t[0] + k[r, 1] * t[1] + k[r, 2] * t[2]
    return P


def project(pts, pose, K, H, W):
    """-> u, v, z (fp64) and valid of every point."""
    p = np.asarray(pts, dtype=np.float64)
    P = combined_matrix(pose, K)
    x = [P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1] + P[r, 2] * p[:, 2] + P[r, 3] for r in range(3)]
    with np.errstate(all="ignore"):
        z = x[2]
        u, v = x[0] / z, x[1] / z
        valid = (u >= 0) & (v >= 0) & (u < W) & (v < H) & (z > 0)
    return u, v, z, valid


def _compact(flags, cap):
    where = np.nonzero(flags)[0].astype(np.int64)
    total = len(where)
    idx = np.zeros(cap, dtype=np.int64)
    idx[:min(total, cap)] = where[:cap]
    return idx, total


def select_visible(pts, poses, K, H, W, cap=None):
    """-> mask (N) bool, idx (cap) int64, info (4) int32."""
    N = len(pts)
    cap = N if cap is None else cap
    mask = np.zeros(N, dtype=bool)
    for pose in poses:
        mask |= project(pts, pose, K, H, W)[3]
    idx, total = _compact(mask, cap)
    return mask, idx, np.array([min(total, cap), total, total > cap, 0], dtype=np.int32)


def build_pairs(pts, pose, K, H, W, stride, thr, depth, depth_points=False, cap=None):
    """-> dict of the outputs of nlg_build_pairs."""
    N = len(pts)
    cap = N if cap is None else cap
    u, v, z, valid = project(pts, pose, K, H, W)
    depth = np.asarray(depth, dtype=np.float64)
    d = np.zeros(N)
    vi = np.nonzero(valid)[0]
    d[vi] = depth[vi] if depth_points else depth[np.trunc(v[vi]).astype(np.int64), np.trunc(u[vi]).astype(np.int64)]
    with np.errstate(all="ignore"):
        us, vs = u / stride, v / stride
        pos = valid & (np.abs(d - z) < thr)
    fallback = int(pos.sum() < MIN_POSITIVES)
    chosen = valid if fallback else pos
    gt_j = np.full(N, -1, dtype=np.int32)
    ci = np.nonzero(chosen)[0]
    gt_j[ci] = (np.trunc(us[ci]) + np.trunc(vs[ci]) * (W // stride)).astype(np.int32)
    i_ids, total = _compact(chosen, cap)
    n = min(total, cap)
    pairs = np.zeros((2, cap), dtype=np.int64)
    pairs[0] = i_ids
    pairs[1, :n] = gt_j[i_ids[:n]]
    with np.errstate(all="ignore"):
        proj = np.stack([us, vs], axis=1).astype(np.float32)
        zf = z.astype(np.float32)
    return {"proj": proj, "z": zf, "proj64": np.stack([us, vs], axis=1), "z64": z, "valid": valid, "pos": pos, "gt_j": gt_j, "pairs": pairs,
            "info": np.array([n, total, total > cap, fallback], dtype=np.int32)}


def conf_target(gt_j, M, dtype=np.float32, rows=None):
    gt_j = np.asarray(gt_j)
    begin, end = (0, len(gt_j)) if rows is None else rows
    out = np.zeros((end - begin, M), dtype=dtype)
    for r, j in enumerate(gt_j[begin:end]):
        if 0 <= j < M:
            out[r, j] = 1
    return out


def cell_grid(Hc, Wc, scale=1.0):
    y, x = np.divmod(np.arange(Hc * Wc), Wc)
    return np.stack([x.astype(np.float32) * np.float32(scale), y.astype(np.float32) * np.float32(scale)], axis=1)
