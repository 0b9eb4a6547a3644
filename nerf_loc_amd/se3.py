"""se(3) exponential and logarithm in differentiable torch, in the convention PoseOptimizer uses (include/nerfloc_refine.h states it: a 6-vector
[log-translation | log-rotation] <-> a column-vector camera-to-world 4 x 4 matrix, the transpose of PyTorch3D's layout; the SQUARED rotation angle is clamped at
1e-4, so below an angle of 0.01 no gradient flows through the angle; the logarithm extrapolates acos linearly beyond |cos| = 1 - 1e-4 and takes a Taylor factor
where |sin| <= 0.5e-4).  Written from that contract; runs on any device and dtype; the HIP library's nlr_se3_* are the same maps in fp64 on the device.
The logarithm does not check the bottom row of its input (that check would read a value back from the device)."""
from __future__ import annotations

import math

import torch

EPS = 1e-4
COS_BOUND = 1e-4


def _hat(w: torch.Tensor) -> torch.Tensor:
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)


def _angle_parts(w: torch.Tensor, eps: float):
    """th (clamped), K = hat(w), K2 = K K."""
    th = torch.clamp((w * w).sum(-1), eps).sqrt()
    K = _hat(w)
    return th, K, K @ K


def _v_matrix(th, K, K2):
    eye = torch.eye(3, dtype=K.dtype, device=K.device)
    a = (1 - torch.cos(th)) / th ** 2
    b = (th - torch.sin(th)) / th ** 3
    return eye + a[:, None, None] * K + b[:, None, None] * K2


def se3_exp_map(log_transform: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """(N, 6) -> (N, 4, 4)."""
    if log_transform.ndim != 2 or log_transform.shape[1] != 6:
        raise ValueError("Expected input to be of shape (N, 6).")
    u, w = log_transform[:, :3], log_transform[:, 3:]
    th, K, K2 = _angle_parts(w, eps)
    inv = 1.0 / th
    f1 = inv * torch.sin(th)
    f2 = inv * inv * (1.0 - torch.cos(th))
    eye = torch.eye(3, dtype=K.dtype, device=K.device)
    R = eye - f1[:, None, None] * K + f2[:, None, None] * K2    # the transpose of I + f1 K + f2 K2: K is skew, K2 symmetric
    t = (_v_matrix(th, K, K2) @ u[:, :, None])
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=K.dtype, device=K.device).expand(u.shape[0], 1, 4)
    return torch.cat([torch.cat([R, t], 2), bottom], 1)


def _acos_linear_extrapolation(x: torch.Tensor, bound: float) -> torch.Tensor:
    slope = -1.0 / math.sqrt(1.0 - bound * bound)
    lo = (x + bound) * slope + math.acos(-bound)
    hi = (x - bound) * slope + math.acos(bound)
    inner = torch.acos(torch.clamp(x, -bound, bound))   # (the clamp keeps acos and its derivative finite on the branch that is not taken)
    return torch.where(x <= -bound, lo, torch.where(x >= bound, hi, inner))


def se3_log_map(transform: torch.Tensor, eps: float = EPS, cos_bound: float = COS_BOUND) -> torch.Tensor:
    """(N, 4, 4) -> (N, 6)."""
    if transform.ndim != 3 or transform.shape[1:] != (4, 4):
        raise ValueError("Input tensor shape has to be (N, 4, 4).")
    R = transform[:, :3, :3].transpose(1, 2)
    c = ((R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]) - 1.0) * 0.5
    phi = _acos_linear_extrapolation(c, 1.0 - cos_bound)
    s = torch.sin(phi)
    ok = s.abs() > 0.5 * eps
    fac = torch.where(ok, phi / (2.0 * torch.where(ok, s, torch.ones_like(s))), 0.5 + phi * phi * (1.0 / 12))
    w = fac[:, None] * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    th, K, K2 = _angle_parts(w, eps)
    u = torch.linalg.solve(_v_matrix(th, K, K2), transform[:, :3, 3:])[:, :, 0]
    return torch.cat([u, w], 1)
