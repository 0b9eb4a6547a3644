"""The synthetic scenes of the absolute-pose tests (tests/test_pnp_cpu.py, tests/test_gpu_pnp.py, tools/pnp_bench.py): a pinhole camera with a known world-to-camera
pose, M matches of pixels and world points, some of them outliers.  Everything comes from numpy.random.default_rng(seed), drawn in the order of `make_scene`."""
from collections import namedtuple

import numpy as np

WIDTH, HEIGHT = 640, 480
K = (500.0, 500.0, 320.0, 240.0)   # fx, fy, cx, cy

Case = namedtuple("Case", "M frac sigma H thr")
CASES = {
    "min4": Case(4, 0.0, 0.0, 64, 8.0),
    "clean65": Case(65, 0.0, 0.0, 64, 8.0),      # one match past a wave
    "half": Case(256, 0.5, 0.5, 256, 8.0),
    "hard": Case(1024, 0.7, 0.5, 1024, 8.0),     # the shipped match count
    "tight": Case(300, 0.3, 0.25, 256, 2.0),
}
NOISE_FREE = ("min4", "clean65")
# ground-truth bars: (degrees, scene units of the camera centre)
GT_BARS = {"min4": (1e-3, 1e-4), "clean65": (1e-3, 1e-4), "half": (0.1, 1e-2), "hard": (0.1, 1e-2), "tight": (0.1, 1e-2)}


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx


def make_scene(M, frac, sigma, seed=0):
    """dict: pts2d (M, 2) fp32, pts3d (M, 3) fp32, R (3, 3), t (3,) world to camera in fp64, is_outlier (M,) bool."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    R = rodrigues(0.3 * rng.normal(size=3))
    t = np.array([0.1, -0.2, 0.3]) + 0.1 * rng.normal(size=3)
    px = rng.uniform(size=(M, 2)) * np.array([WIDTH, HEIGHT])
    depth = rng.uniform(2.0, 8.0, size=M)
    cam = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], axis=1)
    world = (cam - t) @ R            # R^T (cam - t)
    obs = px + sigma * rng.normal(size=(M, 2))
    n_out = int(round(frac * M))
    is_out = np.zeros(M, dtype=bool)
    if n_out:
        which = rng.permutation(M)[:n_out]
        is_out[which] = True
        obs[which] = rng.uniform(size=(n_out, 2)) * np.array([WIDTH, HEIGHT])
    return {"pts2d": obs.astype(np.float32), "pts3d": world.astype(np.float32), "R": R, "t": t, "is_outlier": is_out}


def make_case(name, seed=0):
    c = CASES[name]
    s = make_scene(c.M, c.frac, c.sigma, seed)
    s["case"] = c
    return s


def pose_error(P, R, t):
    """(degrees, distance of the camera centres) between a (12,) / (3, 4) world-to-camera pose and the ground truth."""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    Re, te = P[:, :3], P[:, 3]
    cosang = np.clip((np.trace(Re @ R.T) - 1) / 2, -1, 1)
    # asin of the skew part's size resolves small angles, where acos loses half the digits
    S = Re @ R.T
    sin_ang = 0.5 * np.linalg.norm([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])
    ang = np.degrees(np.arctan2(sin_ang, cosang))
    return ang, float(np.linalg.norm(-Re.T @ te + R.T @ t))
