"""The absolute-pose solver of csrc/pnp.hip restated in fp64 numpy, step by step (include/nerfloc_render.h states the contract): the Philox samples, the P3P
minimal solver, the integer inlier score, the selection, the local optimisation and the result.  The expressions are written in the device code's order of
operations, so that with -ffp-contract=off the two agree to rounding (libm's cos / acos / cbrt / sin aside).

P3P: Grunert's formulation.  With unit bearings j1..j3, world points X1..X3, squared side lengths a2 = |X2 X3|^2, b2 = |X1 X3|^2, c2 = |X1 X2|^2 (divided by b2), cosines
ca = j2.j3, cb = j1.j3, cg = j1.j2 and depths s2 = u s1, s3 = v s1, the law of cosines gives three equations; their difference gives u = N(v) / D(v) with N quadratic
and D linear, and what remains is the quartic N^2 - 2 cg N D + G D^2 = 0 in v, G = 1 - c2 q, q = 1 + v^2 - 2 cb v.  The quartic is solved in closed form (Ferrari: one
real root of the resolvent cubic by Cardano's or the trigonometric formula and one Newton step, then two quadratics), every real root with positive u, v gives depths
(s1 = sqrt(b2 / q)), ONE Newton step on the three law-of-cosines equations polishes them, and the pose follows from the two congruent triangles.
"""
import math

import numpy as np

from tests.sct_dropout_ref import philox4x32_10

LO_ROUNDS, GN_ITERS = 3, 5      # NL_PNP_LO_ROUNDS, NL_PNP_GN_ITERS
TAG = 0x504E50
DAMP = 1e-12
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)


# ------------------------------------------------------------------------------------------ 1. samples
def samples(seed, b, H, M):
    """(H, 3) int32: sample h of problem b; a pure function of (seed, b, h, M).  M < 3: all -1."""
    if M < 3:
        return np.full((H, 3), -1, dtype=np.int32)
    h = np.arange(H, dtype=np.int64)
    w0, w1, w2, _ = philox4x32_10(h, 0, b, TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    i0 = (w0.astype(np.uint64) * np.uint64(M)) >> np.uint64(32)
    j1 = (w1.astype(np.uint64) * np.uint64(M - 1)) >> np.uint64(32)
    j2 = (w2.astype(np.uint64) * np.uint64(M - 2)) >> np.uint64(32)
    i0, j1, j2 = i0.astype(np.int64), j1.astype(np.int64), j2.astype(np.int64)
    i1 = j1 + (j1 >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = j2 + (j2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------ 2. minimal solver
def bearings(px, K):
    fx, fy, cx, cy = K
    bx, by = (px[..., 0] - cx) / fx, (px[..., 1] - cy) / fy
    inv = 1.0 / np.sqrt(bx * bx + by * by + 1.0)
    return np.stack([bx * inv, by * inv, inv], axis=-1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cubic_root(c2, c1, c0):
    """The largest real root of m^3 + c2 m^2 + c1 m + c0, then one Newton step."""
    with np.errstate(all="ignore"):
        sh = c2 / 3.0
        P = c1 - c2 * sh
        Q = 2.0 * sh * sh * sh - sh * c1 + c0
        hq = -0.5 * Q
        D = hq * hq + P * P * P / 27.0
        sD = np.sqrt(np.where(D > 0, D, 0.0))
        t_one = np.cbrt(hq + sD) + np.cbrt(hq - sD)
        rr = np.sqrt(np.where(P < 0, -P / 3.0, 0.0))
        arg = np.clip(hq / (rr * rr * rr), -1.0, 1.0)
        t_three = np.where(rr > 0, 2.0 * rr * np.cos(np.arccos(arg) / 3.0), 0.0)
        m = np.where(D > 0, t_one, t_three) - sh
        f = ((m + c2) * m + c1) * m + c0
        df = (3.0 * m + 2.0 * c2) * m + c1
        step = f / df
        return np.where(np.isfinite(step), m - step, m)


def _quartic_roots(A):
    """A: (..., 5) ascending coefficients.  -> roots (..., 4), real (..., 4) bool."""
    with np.errstate(all="ignore"):
        a, b, c, d = A[..., 3] / A[..., 4], A[..., 2] / A[..., 4], A[..., 1] / A[..., 4], A[..., 0] / A[..., 4]
        a4 = 0.25 * a
        p = b - 6.0 * a4 * a4
        q = c - 2.0 * a4 * b + 8.0 * a4 * a4 * a4
        r = d - a4 * c + a4 * a4 * b - 3.0 * a4 * a4 * a4 * a4
        m = _cubic_root(p, 0.25 * p * p - r, -0.125 * q * q)
        ferrari = m > 0
        s = np.sqrt(np.where(ferrari, 2.0 * m, 1.0))
        hq = q / (2.0 * s)
        base = 0.5 * p + m
        # Ferrari: y^2 + s y + (base - hq) = 0 and y^2 - s y + (base + hq) = 0;  biquadratic (q = 0, m = 0): y^2 = (-p +- sqrt(p^2 - 4 r)) / 2
        d1 = s * s - 4.0 * (base - hq)
        d2 = s * s - 4.0 * (base + hq)
        db = p * p - 4.0 * r
        sdb = np.sqrt(np.where(db >= 0, db, 0.0))
        z1, z2 = 0.5 * (-p + sdb), 0.5 * (-p - sdb)
        sd1, sd2 = np.sqrt(np.where(d1 >= 0, d1, 0.0)), np.sqrt(np.where(d2 >= 0, d2, 0.0))
        sz1, sz2 = np.sqrt(np.where(z1 >= 0, z1, 0.0)), np.sqrt(np.where(z2 >= 0, z2, 0.0))
        yf = np.stack([0.5 * (-s + sd1), 0.5 * (-s - sd1), 0.5 * (s + sd2), 0.5 * (s - sd2)], axis=-1)
        rf = np.stack([d1 >= 0, d1 >= 0, d2 >= 0, d2 >= 0], axis=-1)
        yb = np.stack([sz1, -sz1, sz2, -sz2], axis=-1)
        rb = np.stack([z1 >= 0, z1 >= 0, z2 >= 0, z2 >= 0], axis=-1) & (db >= 0)[..., None]
        y = np.where(ferrari[..., None], yf, yb)
        real = np.where(ferrari[..., None], rf, rb)
        return y - a4[..., None], real


def p3p(j, X):
    """j, X: (H, 3, 3) unit bearings and world points of the samples -> poses (H, 4, 12) (invalid slots zero), nsol (H,) int32."""
    H = j.shape[0]
    poses = np.zeros((H, 4, 12))
    nsol = np.zeros(H, dtype=np.int32)
    with np.errstate(all="ignore"):
        j1, j2, j3 = j[:, 0], j[:, 1], j[:, 2]
        X1, X2, X3 = X[:, 0], X[:, 1], X[:, 2]
        e1, e2, e3 = X2 - X1, X3 - X1, X3 - X2
        c2r, b2r, a2r = _dot(e1, e1), _dot(e2, e2), _dot(e3, e3)
        n = _cross(e1, e2)
        nn = _dot(n, n)
        cg, cb, ca = _dot(j1, j2), _dot(j1, j3), _dot(j2, j3)
        ok = (nn > 1e-12 * c2r * b2r) & (a2r > 0) & (1.0 - cg * cg > 1e-14) & (1.0 - cb * cb > 1e-14) & (1.0 - ca * ca > 1e-14)
        a2, c2 = a2r / b2r, c2r / b2r
        k = c2 - a2
        n0, n1, n2 = k - 1.0, -2.0 * cb * k, 1.0 + k
        d0, d1 = -2.0 * cg, 2.0 * ca
        g0, g1, g2 = 1.0 - c2, 2.0 * c2 * cb, -c2
        D0, D1, D2 = d0 * d0, 2.0 * d0 * d1, d1 * d1
        tc = 2.0 * cg
        A = np.stack([n0 * n0 - tc * (n0 * d0) + g0 * D0,
                      2.0 * n0 * n1 - tc * (n0 * d1 + n1 * d0) + (g0 * D1 + g1 * D0),
                      (2.0 * n0 * n2 + n1 * n1) - tc * (n1 * d1 + n2 * d0) + (g0 * D2 + g1 * D1 + g2 * D0),
                      2.0 * n1 * n2 - tc * (n2 * d1) + (g1 * D2 + g2 * D1),
                      n2 * n2 + g2 * D2], axis=-1)
        roots, real = _quartic_roots(A)
        r1 = _cross(e2, n) / nn[:, None]
        r2 = _cross(n, e1) / nn[:, None]
        r3 = n / nn[:, None]
        for kk in range(4):
            v = roots[:, kk]
            qv = 1.0 + v * v - 2.0 * cb * v
            s1 = np.sqrt(b2r / qv)
            u = ((n2 * v + n1) * v + n0) / (d1 * v + d0)
            s2, s3 = u * s1, v * s1
            # one Newton step on F(s) = (s1^2 + s2^2 - 2 s1 s2 cg - c2, s1^2 + s3^2 - 2 s1 s3 cb - b2, s2^2 + s3^2 - 2 s2 s3 ca - a2), by Cramer's rule
            F1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2r
            F2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2r
            F3 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2r
            J11, J12 = 2.0 * (s1 - s2 * cg), 2.0 * (s2 - s1 * cg)
            J21, J23 = 2.0 * (s1 - s3 * cb), 2.0 * (s3 - s1 * cb)
            J32, J33 = 2.0 * (s2 - s3 * ca), 2.0 * (s3 - s2 * ca)
            det = -J11 * (J23 * J32) - J12 * (J21 * J33)
            ds1 = (-F1 * (J23 * J32) - J12 * (F2 * J33 - J23 * F3)) / det
            ds2 = (J11 * (F2 * J33 - J23 * F3) - F1 * (J21 * J33)) / det
            ds3 = (J11 * (-F2 * J32) - J12 * (J21 * F3) + F1 * (J21 * J32)) / det
            step_ok = np.isfinite(ds1) & np.isfinite(ds2) & np.isfinite(ds3)
            s1 = np.where(step_ok, s1 - ds1, s1)
            s2 = np.where(step_ok, s2 - ds2, s2)
            s3 = np.where(step_ok, s3 - ds3, s3)
            Y1, Y2, Y3 = s1[:, None] * j1, s2[:, None] * j2, s3[:, None] * j3
            y1, y2 = Y2 - Y1, Y3 - Y1
            ny = _cross(y1, y2)
            R = y1[:, :, None] * r1[:, None, :] + y2[:, :, None] * r2[:, None, :] + ny[:, :, None] * r3[:, None, :]
            t = Y1 - (R[:, :, 0] * X1[:, 0:1] + R[:, :, 1] * X1[:, 1:2] + R[:, :, 2] * X1[:, 2:3])
            pose = np.concatenate([R, t[:, :, None]], axis=2).reshape(H, 12)
            good = ok & real[:, kk] & (v > 0) & (u > 0) & (s1 > 0) & (s2 > 0) & (s3 > 0) & np.isfinite(pose).all(axis=1)
            for h in np.nonzero(good)[0]:
                poses[h, nsol[h]] = pose[h]
                nsol[h] += 1
    return poses, nsol


def hypotheses(pts2d, pts3d, K, seed, b, H):
    """Steps 1 + 2 of one problem: (samples (H, 3), poses (H, 4, 12), nsol (H,)).  M < 4: nsol = 0."""
    M = len(pts2d)
    idx = samples(seed, b, H, M)
    if M < 4:
        return idx, np.zeros((H, 4, 12)), np.zeros(H, dtype=np.int32)
    p2, p3 = pts2d.astype(np.float64), pts3d.astype(np.float64)
    poses, nsol = p3p(bearings(p2[idx], K), p3[idx])
    return idx, poses, nsol


# ------------------------------------------------------------------------------------------ 3. score
def reproject(pose, pts2d, pts3d, K):
    """pose (..., 12) against all matches -> (e2 (..., M), z (..., M)) in fp64."""
    fx, fy, cx, cy = K
    P = np.asarray(pose, dtype=np.float64)[..., None, :]
    X = pts3d.astype(np.float64)
    x = pts2d.astype(np.float64)
    with np.errstate(all="ignore"):
        xc = P[..., 0] * X[:, 0] + P[..., 1] * X[:, 1] + P[..., 2] * X[:, 2] + P[..., 3]
        yc = P[..., 4] * X[:, 0] + P[..., 5] * X[:, 1] + P[..., 6] * X[:, 2] + P[..., 7]
        zc = P[..., 8] * X[:, 0] + P[..., 9] * X[:, 1] + P[..., 10] * X[:, 2] + P[..., 11]
        du = fx * (xc / zc) + cx - x[:, 0]
        dv = fy * (yc / zc) + cy - x[:, 1]
        return du * du + dv * dv, zc


def inlier_mask(pose, pts2d, pts3d, K, thr):
    e2, z = reproject(pose, pts2d, pts3d, K)
    with np.errstate(invalid="ignore"):
        return (z > 0) & (e2 <= thr * thr)


def margin(pose, pts2d, pts3d, K, thr):
    """The closest any e2 of points in front of the camera comes to thr^2, relative: the precondition of comparing integer counts exactly."""
    e2, z = reproject(pose, pts2d, pts3d, K)
    with np.errstate(invalid="ignore"):
        rel = np.abs(e2 / (thr * thr) - 1.0)
    rel = rel[np.isfinite(rel) & (z > 0)]
    return float(rel.min()) if rel.size else np.inf


def score(poses, valid, pts2d, pts3d, K, thr):
    """poses (P, 12), valid (P,) bool -> (P,) int32 counts; an invalid slot or a pose with a non-finite entry scores -1."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    cnt = inlier_mask(poses, pts2d, pts3d, K, thr).sum(axis=-1).astype(np.int32) if len(pts2d) else np.zeros(len(poses), dtype=np.int32)
    cnt[~(np.asarray(valid, dtype=bool) & np.isfinite(poses).all(axis=1))] = -1
    return cnt


def slot_valid(nsol):
    return (np.arange(4)[None, :] < np.asarray(nsol)[:, None]).reshape(-1)


# ------------------------------------------------------------------------------------------ 4. selection
def select(counts):
    """(best candidate, best count): the highest count, among equals the lowest index."""
    best = int(np.argmax(counts))   # numpy's argmax returns the first maximum
    return best, int(counts[best])


# ------------------------------------------------------------------------------------------ 5. local optimisation
def _mul3(A, B):
    """A B for 3 x 3 (or 3 x n) operands as explicit sums in the device's order (no BLAS: its order of operations, and its use of fused multiply-adds, vary)."""
    return A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :] + A[:, 2:3] * B[2:3, :]


def _exp_so3(w):
    w = [float(v) for v in w]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th2 < 1e-16:
        A, B = 1.0, 0.5
    else:
        th = math.sqrt(th2)
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2   # libm's, not a vectorised variant that may differ by machine
    return np.eye(3) + A * Kx + B * _mul3(Kx, Kx)


def _cholesky_solve(A, g):
    """Solve A d = -g for a 6 x 6 symmetric A by Cholesky; None when a pivot is not positive."""
    n = len(g)
    L = np.zeros((n, n))
    for jj in range(n):
        s = A[jj, jj]
        for c in range(jj):
            s = s - L[jj, c] * L[jj, c]
        if not s > 0:
            return None
        L[jj, jj] = np.sqrt(s)
        for i in range(jj + 1, n):
            a = A[i, jj]
            for c in range(jj):
                a = a - L[i, c] * L[jj, c]
            L[i, jj] = a / L[jj, jj]
    d = np.zeros(n)
    for i in range(n):
        a = -g[i]
        for c in range(i):
            a = a - L[i, c] * d[c]
        d[i] = a / L[i, i]
    for i in reversed(range(n)):
        a = d[i]
        for c in range(i + 1, n):
            a = a - L[c, i] * d[c]
        d[i] = a / L[i, i]
    return d


def gn_step(pose, p2, p3, K):
    """One Gauss-Newton iteration on the given matches (fp64 arrays): the new pose, or None (failed factorisation / non-finite step).  The device sums the normal
    equations per thread and then by a tree; here they are summed match by match: the two differ by the rounding of that sum alone."""
    fx, fy, cx, cy = K
    P = pose.reshape(3, 4)
    R, t = P[:, :3], P[:, 3]
    X, Y, Z = p3[:, 0], p3[:, 1], p3[:, 2]
    yx = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z
    yy = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z
    yz = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z
    xc, yc, zc = yx + t[0], yy + t[1], yz + t[2]
    ru = fx * (xc / zc) + cx - p2[:, 0]
    rv = fy * (yc / zc) + cy - p2[:, 1]
    a, b = fx / zc, -fx * xc / (zc * zc)
    c, d = fy / zc, -fy * yc / (zc * zc)
    zero = np.zeros_like(a)
    Ju = np.stack([b * yy, a * yz - b * yx, -a * yy, a, zero, b], axis=1)
    Jv = np.stack([d * yy - c * yz, -d * yx, c * yx, zero, c, d], axis=1)
    A = (Ju[:, :, None] * Ju[:, None, :] + Jv[:, :, None] * Jv[:, None, :]).sum(axis=0) + DAMP * np.eye(6)
    g = (Ju * ru[:, None] + Jv * rv[:, None]).sum(axis=0)
    step = _cholesky_solve(A, g)
    if step is None or not np.isfinite(step).all():
        return None
    Rn = _mul3(_exp_so3(step[:3]), R)
    new = np.concatenate([Rn, (t + step[3:])[:, None]], axis=1).reshape(12)
    return new if np.isfinite(new).all() else None


def refine(pose, pts2d, pts3d, K, thr, min_inliers=4):
    """Steps 5 + 6 from a given pose -> (pose (12,), mask (M,) bool, num_inliers, success)."""
    M = len(pts2d)
    pose = np.asarray(pose, dtype=np.float64).reshape(12).copy()
    if M < 4 or not np.isfinite(pose).all():
        return IDENTITY.copy(), np.zeros(M, dtype=bool), 0, 0
    p2, p3 = pts2d.astype(np.float64), pts3d.astype(np.float64)
    stop = False
    for _ in range(LO_ROUNDS):
        m = inlier_mask(pose, pts2d, pts3d, K, thr)
        if m.sum() < 4:
            break
        for _ in range(GN_ITERS):
            new = gn_step(pose, p2[m], p3[m], K)
            if new is None:
                stop = True
                break
            pose = new
        if stop:
            break
    mask = inlier_mask(pose, pts2d, pts3d, K, thr)
    n = int(mask.sum())
    return pose, mask, n, int(n >= min_inliers)


# ------------------------------------------------------------------------------------------ the whole
def ransac(pts2d, pts3d, K, thr, H, seed=0, b=0, min_inliers=4):
    """dict: pose, mask, success, num_inliers, best_candidate, best_count, counts (4 H,), samples, poses, nsol."""
    M = len(pts2d)
    idx, poses, nsol = hypotheses(pts2d, pts3d, K, seed, b, H)
    counts = score(poses.reshape(-1, 12), slot_valid(nsol), pts2d, pts3d, K, thr)
    best, best_count = select(counts)
    if M < 4 or best_count < 0:
        pose, mask, n, success = IDENTITY.copy(), np.zeros(M, dtype=bool), 0, 0
    else:
        pose, mask, n, success = refine(poses.reshape(-1, 12)[best], pts2d, pts3d, K, thr, min_inliers)
    return {"pose": pose, "mask": mask, "success": success, "num_inliers": n, "best_candidate": best, "best_count": best_count, "counts": counts, "samples": idx,
            "poses": poses, "nsol": nsol}
