"""The camera pose from the matcher's 2D-3D matches: P3P RANSAC with a fixed number of hypotheses + Gauss-Newton refinement in the HIP library (csrc/pnp.hip,
nl_pnp_ransac), on the stream the matches were produced on.  Replaces the external CPU solver the reference calls (pycolmap.absolute_pose_estimation,
nerf_pose_estimator.py:528-540, 557-583); include/nerfloc_render.h states the algorithm.

`absolute_pose` / `absolute_pose_batch` return DEVICE tensors and never synchronise with the host: the result can feed the next stage (cascade matching) or be
captured in a graph.  `estimate_pose` is the drop-in for NerfPoseEstimator.estimate_pose and returns numpy, so it synchronises, as the reference's does.
Two calls with one seed give the same bits; seed = 0 is the default, so results are reproducible unless the caller varies the seed.  CPU tensors are refused: there
is no CPU fallback, as everywhere in the package.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._packing import require_device

DEFAULT_HYPOTHESES = 1024


def _intrinsics(K):
    """(fx, fy, cx, cy) as host floats from four numbers or a 3 x 3 matrix.  A DEVICE tensor costs one copy to the host, which synchronises: pass numbers or a CPU
    tensor where that matters (inside a graph capture it must be numbers or a CPU tensor)."""
    if torch.is_tensor(K):
        K = K.detach().cpu().double()
        if K.shape == (3, 3):
            return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        K = K.reshape(-1).tolist()
    elif hasattr(K, "shape") and tuple(K.shape) == (3, 3):
        return float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    K = [float(v) for v in K]
    if len(K) != 4:
        raise ValueError("K must be a 3 x 3 matrix or (fx, fy, cx, cy)")
    return tuple(K)


def _matches(pts2d, pts3d):
    require_device("absolute_pose", pts2d, pts3d)
    if pts2d.dim() != 2 or pts2d.shape[1] != 2 or pts3d.dim() != 2 or pts3d.shape[1] != 3 or pts2d.shape[0] != pts3d.shape[0]:
        raise ValueError("absolute_pose: pts2d must be (M, 2) and pts3d (M, 3)")
    if pts2d.device != pts3d.device:
        raise ValueError("absolute_pose: pts2d and pts3d must be on one device")
    return pts2d.detach().float().contiguous(), pts3d.detach().float().contiguous()


def _transforms(pose):
    """(B, 12) world-to-camera rows -> (T_w2c, T_c2w), each (B, 4, 4) float64, by device operations alone."""
    B = pose.shape[0]
    Rt = pose.view(B, 3, 4)
    T = torch.zeros(B, 4, 4, dtype=torch.float64, device=pose.device)
    T[:, :3] = Rt
    T[:, 3, 3] = 1.0
    Ti = torch.zeros_like(T)
    Rinv = Rt[:, :, :3].transpose(1, 2)
    Ti[:, :3, :3] = Rinv
    Ti[:, :3, 3] = -(Rinv @ Rt[:, :, 3:]).squeeze(-1)
    Ti[:, 3, 3] = 1.0
    return T, Ti


def absolute_pose_batch(problems, hypotheses: int = DEFAULT_HYPOTHESES, seed: int = 0, min_inliers: int = 4, precision=None):
    """One library call for all problems.  `problems`: a list of dicts with `pts2d` (M, 2), `pts3d` (M, 3), `K` (3 x 3 or four numbers) and `thr` (pixels), all
    tensors on one HIP device.  Returns a list of dicts of DEVICE tensors: `T_w2c`, `T_c2w` (4 x 4 float64), `inliers` (M,) bool, `num_inliers`, `success`
    (0-d int32), plus `best_candidate`, `best_count`.  Problem b draws the samples of index b: its result does not depend on the other problems.
    `precision` is accepted for symmetry with the other modules; the solver is fp64 throughout, whatever it says."""
    if precision is not None and precision not in _lib.PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}")
    B = len(problems)
    if B == 0:
        return []
    lib = _lib.load()
    pairs = [_matches(p["pts2d"], p["pts3d"]) for p in problems]
    dev = pairs[0][0].device
    if any(a.device != dev for a, _ in pairs):
        raise ValueError("absolute_pose_batch: all problems must be on one device")
    p2 = pairs[0][0] if B == 1 else torch.cat([a for a, _ in pairs])
    p3 = pairs[0][1] if B == 1 else torch.cat([b for _, b in pairs])
    sizes = [int(a.shape[0]) for a, _ in pairs]
    offsets = (C.c_int32 * (B + 1))(0)
    for b, m in enumerate(sizes):
        offsets[b + 1] = offsets[b] + m
    intr = (C.c_double * (4 * B))(*[v for p in problems for v in _intrinsics(p["K"])])
    thr = (C.c_double * B)(*[float(p["thr"]) for p in problems])
    H = int(hypotheses)
    with torch.cuda.device(dev):
        ws = _lib.workspace(lib.nl_pnp_workspace_bytes(offsets[B], B, H), dev, f"absolute_pose: hypotheses must be a multiple of 64 in 64..65536, got {H}", ValueError)
        pose = torch.empty(B, 12, dtype=torch.float64, device=dev)
        mask = torch.empty(max(int(offsets[B]), 1), dtype=torch.uint8, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        st = _lib.stream(dev)
        _lib.check(lib.nl_pnp_ransac(p2.data_ptr(), p3.data_ptr(), offsets, intr, thr, B, H, int(seed) & 0xFFFFFFFFFFFFFFFF, int(min_inliers), pose.data_ptr(),
                                     mask.data_ptr(), info.data_ptr(), None, ws.data_ptr(), ws.numel(), st), "nl_pnp_ransac")
        T, Ti = _transforms(pose)
        inl = mask.bool()
    return [{"T_w2c": T[b], "T_c2w": Ti[b], "inliers": inl[offsets[b]:offsets[b + 1]], "num_inliers": info[b, 1], "success": info[b, 0],
             "best_candidate": info[b, 2], "best_count": info[b, 3]} for b in range(B)]


def absolute_pose(pts2d, pts3d, K, thr, hypotheses: int = DEFAULT_HYPOTHESES, seed: int = 0, min_inliers: int = 4, precision=None):
    """The pose of one camera from M matches: a dict of DEVICE tensors (see absolute_pose_batch), without a host synchronisation when K is numbers or a CPU tensor."""
    return absolute_pose_batch([{"pts2d": pts2d, "pts3d": pts3d, "K": K, "thr": thr}], hypotheses, seed, min_inliers, precision)[0]


def estimate_pose(matched_kps_2d, matched_kps_3d, K, width=None, height=None, ransac_thresh=48, **kw):
    """Drop-in for NerfPoseEstimator.estimate_pose: (T_c2w as a (4, 4) float64 numpy array, inliers as a numpy bool array), or None without success.  `width` and
    `height` are accepted for the reference's signature; the pinhole model does not need them.  Synchronises (it returns numpy).  kw: hypotheses, seed,
    min_inliers."""
    r = absolute_pose(matched_kps_2d, matched_kps_3d, K, ransac_thresh, **kw)
    if int(r["success"]) == 0:
        return None
    return r["T_c2w"].cpu().numpy(), r["inliers"].cpu().numpy()
