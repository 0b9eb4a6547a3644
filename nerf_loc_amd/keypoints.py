"""Drop-ins for the correspondence geometry of the reference's NerfPoseEstimator (models/nerf_pose_estimator.py:126-190 and :487-488) on libnerfloc_geom.so
(include/nerfloc_geom.h): which SfM points the support views see, the 3D-2D pairs of a pose, the dense loss target and the coarse cell grid.

HIP tensors take the library: three launches per call, no host decision.  The `*_padded` forms return fixed-capacity lists with DEVICE-side counts: they never
synchronise and replay from torch.cuda.graph.  The two functions with the reference's return values need the one read-back an exact shape needs.
CPU tensors take the eager formulation below (`eager_*`), written from the header's contract: fp64 from the loaded inputs to every decision, the world-to-camera
map as adjugate / determinant of the pose's affine part.  It is also the comparator of the tests and of tools/geom_bench.py.  HIP tensors of a dtype the library
does not read raise: there is no quiet fall-back.

PREFER_LIBRARY: which drop-in takes the library on HIP tensors; tools/geom_bench.py measures both (README, "Keypoint geometry").
"""
from __future__ import annotations

import torch

from . import _geom_lib

PREFER_LIBRARY = {"select": True, "pairs": True, "target": True}
MIN_POSITIVES = _geom_lib.MIN_POSITIVES
_grid_cache: dict = {}


# ---------------------------------------------------------------------------------------------------------------- the eager formulation
def _stack_poses(poses):
    return poses if torch.is_tensor(poses) else torch.stack(list(poses))


def _combined(poses, K):
    """poses (V, 4, 4), K (3, 3), any float dtype -> K R (V, 3, 3), K t (V, 3) in fp64, [R | t] the inverse of the poses' affine parts (adjugate / determinant)."""
    T, K = poses.to(torch.float64), K.to(torch.float64)
    A, c = T[:, :3, :3], T[:, :3, 3]
    cof = torch.stack([torch.linalg.cross(A[:, 1], A[:, 2]), torch.linalg.cross(A[:, 2], A[:, 0]), torch.linalg.cross(A[:, 0], A[:, 1])], dim=1)
    det = (A[:, 0] * cof[:, 0]).sum(-1)
    R = cof.transpose(1, 2) / det[:, None, None]
    t = -(R @ c[:, :, None])
    return K @ R, (K @ t)[:, :, 0]


def _project(pts, poses, K, H, W):
    """-> u, v, z, valid, each (V, N), fp64."""
    KR, Kt = _combined(poses, K)
    x = pts.to(torch.float64) @ KR.transpose(1, 2) + Kt[:, None, :]
    z = x[..., 2]
    u, v = x[..., 0] / z, x[..., 1] / z
    return u, v, z, (u >= 0) & (v >= 0) & (u < W) & (v < H) & (z > 0)


def _pad(ids, cap):
    out = ids.new_zeros(ids.shape[:-1] + (cap,))
    n = min(cap, ids.shape[-1])
    out[..., :n] = ids[..., :n]
    return out


def eager_select_3d_keypoints(pts3d, poses, K, H, W):
    """The visible indices (exact size) and the mask, in eager torch on the tensors' device."""
    mask = _project(pts3d, _stack_poses(poses), K, H, W)[3].any(dim=0)
    return torch.nonzero(mask).squeeze(1), mask


def eager_build_3d_2d_pairs(pts3d, H, W, K, pose, thr, stride, depth_map=None, depth_points=None):
    """dict(proj, z, valid, pos, gt_j, pairs (2, P) of exact size, used_fallback) in eager torch."""
    u, v, z, valid = (a[0] for a in _project(pts3d, pose[None], K, H, W))
    zero = torch.zeros_like(u)
    if depth_points is not None:
        d = depth_points.to(torch.float64)
    else:
        d = depth_map[torch.where(valid, v, zero).long(), torch.where(valid, u, zero).long()].to(torch.float64)
    pos = valid & ((d - z).abs() < thr)
    fallback = pos.sum() < MIN_POSITIVES
    chosen = torch.where(fallback, valid, pos)
    us, vs = u / stride, v / stride
    cell = torch.where(valid, us, zero).long() + torch.where(valid, vs, zero).long() * (W // stride)
    gt_j = torch.where(chosen, cell, torch.full_like(cell, -1)).to(torch.int32)
    i_ids = torch.nonzero(chosen).squeeze(1)
    return {"proj": torch.stack([us, vs], dim=1).to(torch.float32), "z": z.to(torch.float32), "valid": valid, "pos": pos, "gt_j": gt_j,
            "pairs": torch.stack([i_ids, gt_j[i_ids].to(torch.int64)]), "used_fallback": fallback.to(torch.int32)}


def eager_conf_matrix_target(gt_j, M, dtype=torch.float32):
    """The reference's tensor: zeros plus an index-put (rows whose gt_j is outside [0, M) stay zero)."""
    out = torch.zeros((gt_j.shape[0], M), dtype=dtype, device=gt_j.device)
    rows = torch.nonzero((gt_j >= 0) & (gt_j < M)).squeeze(1)
    out[rows, gt_j[rows].long()] = 1
    return out


def eager_cell_grid(Hc, Wc, scale=1.0, device="cpu"):
    gy, gx = torch.meshgrid(torch.arange(Hc, device=device), torch.arange(Wc, device=device), indexing="ij")
    return torch.stack([gx, gy], dim=-1).reshape(-1, 2).to(torch.float32) * scale


# ---------------------------------------------------------------------------------------------------------------- the drop-ins
def _library(piece, *tensors):
    """True: the library call; False: the eager formulation (CPU tensors, or a piece PREFER_LIBRARY leaves to eager).  Mixed devices raise."""
    cuda = [t.is_cuda for t in tensors if t is not None]
    if any(cuda) and not all(cuda):
        raise ValueError("keypoints: all tensors must be on one device")
    return bool(cuda) and all(cuda) and PREFER_LIBRARY[piece]


def _hip_inputs(pts3d, K, what):
    if pts3d.dtype != torch.float32 or K.dtype != torch.float32:
        raise ValueError(f"{what}: on a HIP device points and K must be fp32 (poses fp32 or fp64)")
    return pts3d.detach().contiguous(), K.detach().contiguous()


def select_3d_keypoints_padded(pts3d, poses, K, H, W, capacity=None):
    """-> idx (capacity, default N) int64 ascending with zeros behind the count, mask (N) bool, num and overflow (0-dim int32, on the device).  No synchronisation."""
    poses = _stack_poses(poses)
    cap = int(pts3d.shape[0] if capacity is None else capacity)
    if _library("select", pts3d, poses, K):
        pts, Kc = _hip_inputs(pts3d, K, "select_3d_keypoints")
        mask, idx, info = _geom_lib.select_visible(pts, poses.detach().contiguous(), Kc, H, W, cap)
        return idx, mask, info[0], info[2]
    ids, mask = eager_select_3d_keypoints(pts3d, poses, K, H, W)
    total = torch.tensor(ids.shape[0], dtype=torch.int32, device=pts3d.device)
    return _pad(ids, cap), mask, total.clamp(max=cap), (total > cap).to(torch.int32)


def select_3d_keypoints(pts3d, poses, K, H, W):
    """The reference's select_3d_keypoints: the ascending int64 indices of the points at least one pose sees.  poses: a list of (4, 4) tensors or (V, 4, 4)."""
    poses = _stack_poses(poses)
    if _library("select", pts3d, poses, K):
        idx, _, num, _ = select_3d_keypoints_padded(pts3d, poses, K, H, W)
        return idx[:int(num)]   # the one read-back
    return eager_select_3d_keypoints(pts3d, poses, K, H, W)[0]


def cell_grid(Hc, Wc, scale=1.0, device="cpu"):
    """(Hc Wc, 2) fp32 cell coordinates (x, y) * scale, from a per-(shape, scale, device) cache: treat it as read-only."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (int(Hc), int(Wc), float(scale), dev)
    if key not in _grid_cache:
        _grid_cache[key] = _geom_lib.cell_grid(Hc, Wc, scale, dev) if dev.type == "cuda" else eager_cell_grid(Hc, Wc, scale, dev)
    return _grid_cache[key]


def pts2d_grid(H, W, stride, device="cpu"):
    """The reference's pts2d_grid: (H // stride * W // stride, 2) int64, x then y; cached like cell_grid."""
    dev = cell_grid(H // stride, W // stride, 1.0, device).device
    key = (H // stride, W // stride, "int64", dev)
    if key not in _grid_cache:
        _grid_cache[key] = cell_grid(H // stride, W // stride, 1.0, dev).to(torch.int64)
    return _grid_cache[key]


def build_3d_2d_pairs_padded(pts3d, H, W, K, pose, thr, stride, depth_map=None, depth_points=None, capacity=None):
    """-> dict(pairs (2, capacity, default N) int64 with zeros behind the count, gt_j (N) int32, proj (N, 2), z (N), valid, pos (N) bool, and on the device num,
    overflow, used_fallback (0-dim int32)).  Exactly one of depth_map (H, W) / depth_points (N).  No synchronisation."""
    if (depth_map is None) == (depth_points is None):
        raise ValueError("build_3d_2d_pairs: exactly one of depth_map and depth_points")
    if H % stride or W % stride:
        raise ValueError("build_3d_2d_pairs: stride must divide H and W")
    cap = int(pts3d.shape[0] if capacity is None else capacity)
    depth = depth_map if depth_points is None else depth_points
    if _library("pairs", pts3d, pose, K, depth):
        pts, Kc = _hip_inputs(pts3d, K, "build_3d_2d_pairs")
        if depth.dtype != torch.float32:
            raise ValueError("build_3d_2d_pairs: on a HIP device the depth source must be fp32")
        out = _geom_lib.build_pairs(pts, pose.detach().contiguous(), Kc, H, W, stride, thr, depth.detach().contiguous(), depth_points is not None, cap)
        info = out.pop("info")
        out.update(num=info[0], overflow=info[2], used_fallback=info[3])
        return out
    out = eager_build_3d_2d_pairs(pts3d, H, W, K, pose, thr, stride, depth_map, depth_points)
    total = torch.tensor(out["pairs"].shape[1], dtype=torch.int32, device=pts3d.device)
    out.update(pairs=_pad(out["pairs"], cap), num=total.clamp(max=cap), overflow=(total > cap).to(torch.int32))
    return out


def build_3d_2d_pairs(pts3d, H, W, K, pose, thr, stride, depth_map=None, depth_points=None):
    """The reference's build_3d_2d_pairs -> (pts3d, pts2d_grid, pts3d_proj, pos_pairs); depth_points (N) stands for its depth-from-the-renderer branch."""
    out = build_3d_2d_pairs_padded(pts3d, H, W, K, pose, thr, stride, depth_map, depth_points)
    return pts3d, pts2d_grid(H, W, stride, pts3d.device), out["proj"], out["pairs"][:, :int(out["num"])]


def conf_matrix_target(gt_j, M, dtype=torch.float32):
    """The dense (N, M) matching target of gt_j (N) int32 (build_3d_2d_pairs_padded): fp32 is what S2DMatching's training forward reads without a conversion copy,
    torch.int64 is the reference's conf_matrix_gt."""
    if dtype not in (torch.float32, torch.int64):
        raise ValueError("conf_matrix_target: dtype is torch.float32 or torch.int64")
    if _library("target", gt_j):
        if gt_j.dtype != torch.int32:
            raise ValueError("conf_matrix_target: on a HIP device gt_j must be int32")
        return _geom_lib.conf_target(gt_j.contiguous(), M, dtype)
    return eager_conf_matrix_target(gt_j, M, dtype)
