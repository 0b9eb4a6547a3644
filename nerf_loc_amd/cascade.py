"""Cascade localisation (the reference's `cascade_matching`, models/nerf_pose_estimator.py:329-348) as one linear chain of launches: the first matcher's pose selects
the 3-D points it sees, a second matcher runs on those points alone, and the number of selected points never leaves the device.

    stage one     matcher.localize(data, K, thr, ...)                                           descriptors -> pose, no read-back (matcher.py)
    selection     keypoints.select_3d_keypoints_padded(kps3d, T_c2w[None], K, H, W)             idx (N) with zeros behind the count, num on the device
    gather        index_select of desc_3d, pos_emd_3d, desc_3d_fine, kps3d by idx               rows behind the count gather row 0: finite, and ignored
    stage two     matcher_fine.localize(gathered, K, thr, ..., num_points=num)                  libnerfloc_counted.so: only the first num rows exist
    the rule      T = stage two's if num > 0 else stage one's                                   (`if len(select_idx) > 0`), chosen on the device

Stage two's pose is the identity when it fails (fewer than four matches, too few inliers), as the reference's `estimate` returns np.eye(4).  Every result is a
device tensor; after one warm call (weight images, the cached intrinsics) the function makes no host synchronisation, uses no side stream and replays from
torch.cuda.graph.  The exact-size composition it replaces — localize, select_3d_keypoints, indexing, forward, absolute_pose — reads back four times per cascade;
README.md gives both ways' measured times and says which to prefer when.  Eval mode on HIP tensors only.
"""
from __future__ import annotations

import torch

from . import keypoints
from .pose import DEFAULT_HYPOTHESES, _intrinsics

POINT_KEYS = ("desc_3d", "pos_emd_3d", "desc_3d_fine", "kps3d")   # the per-3-D-point inputs of Matcher.forward: what the selection gathers
_k_cache: dict = {}


_K_CACHE_MAX = 16


def _device_K(K, device):
    """The (3, 3) fp32 intrinsics on `device`, uploaded once per (values, device): an upload synchronises and cannot be captured, so the FIRST call with new
    intrinsics is the warm call, whatever else is warm.  The cache holds the last _K_CACHE_MAX cameras (oldest out first); a caller whose intrinsics change per
    frame pays the upload per frame and should pass K_device instead."""
    fx, fy, cx, cy = _intrinsics(K)
    key = (fx, fy, cx, cy, device)
    if key not in _k_cache:
        if len(_k_cache) >= _K_CACHE_MAX:
            del _k_cache[next(iter(_k_cache))]
        _k_cache[key] = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32).to(device)
    return _k_cache[key]


_n_cache: dict = {}


def _device_count(n, device):
    """The constant n as a 0-d int32 tensor on `device`, uploaded once per (n, device) like the intrinsics."""
    key = (n, device)
    if key not in _n_cache:
        if len(_n_cache) >= _K_CACHE_MAX:
            del _n_cache[next(iter(_n_cache))]
        _n_cache[key] = torch.tensor(n, dtype=torch.int32).to(device)
    return _n_cache[key]


@torch.no_grad()
def localize_cascade(matcher, matcher_fine, data, K, H, W, thr, hypotheses: int = DEFAULT_HYPOTHESES, seed: int = 0, min_inliers: int = 4, K_device=None):
    """The two-stage cascade.  matcher, matcher_fine: two `Matcher`s in eval mode; data: what Matcher.localize reads; K: (fx, fy, cx, cy) or a 3 x 3 matrix as
    numbers or a CPU tensor (the solver's host copy); K_device (optional): the same intrinsics as a (3, 3) fp32 tensor on the inputs' device, prepared by the
    caller — without it the device copy comes from a small cache, uploaded on the first call with these values (see _device_K); H, W: the image bounds of the visibility selection, in pixels; thr, hypotheses, seed, min_inliers: both stages' solver settings.
    Returns DEVICE tensors: T_c2w, T_w2c (4 x 4 float64) by the reference's rule, num_points (0-d int32: the points stage one's pose sees), stage (0-d int32: 2 if
    num_points > 0 else 1), idx (N) int64 and the two stages' `localize` dicts as stage1 and stage2.  With num_points = n, stage2 equals matcher_fine.forward and
    pose.absolute_pose on the first n gathered rows, bit for bit."""
    if matcher.training or matcher_fine.training:
        raise RuntimeError("localize_cascade: eval mode only (training goes through Matcher.forward)")
    pts = data["kps3d"]
    if not all(torch.is_tensor(data[k]) and data[k].is_cuda for k in POINT_KEYS):
        raise ValueError("localize_cascade: the inputs must be HIP tensors (there is no CPU fallback)")
    if torch.is_tensor(K) and K.is_cuda:
        raise ValueError("localize_cascade: K must be numbers or a CPU tensor (a device tensor would synchronise)")
    dev = pts.device
    # Stage one takes the counted path too, with the count N (the bits of the call without a count): its selection then reads maxima that a KERNEL cleared
    # (nlk_s2d_select_counted).  nl_s2d_match clears its own with a memset node, and replayed from a captured graph a cascade whose stage one used that selection
    # was seen to lose matches now and then; its scores, which is all the counted path takes from it, were always right.
    s1 = matcher.localize(data, K, thr, hypotheses=hypotheses, seed=seed, min_inliers=min_inliers, num_points=_device_count(int(pts.shape[0]), dev))
    pts32 = pts.detach().to(torch.float32).contiguous()
    if K_device is not None and (not torch.is_tensor(K_device) or K_device.device != dev or K_device.dtype != torch.float32 or tuple(K_device.shape) != (3, 3)):
        raise ValueError("localize_cascade: K_device must be a (3, 3) fp32 tensor on the inputs' device")
    Kd = _device_K(K, dev) if K_device is None else K_device
    idx, _, num, _ = keypoints.select_3d_keypoints_padded(pts32, s1["T_c2w"][None], Kd, int(H), int(W))
    sub = dict(data)
    for k in POINT_KEYS:
        sub[k] = data[k].index_select(0, idx)
    s2 = matcher_fine.localize(sub, K, thr, hypotheses=hypotheses, seed=seed, min_inliers=min_inliers, num_points=num)
    two = num > 0
    return {"T_c2w": torch.where(two, s2["T_c2w"], s1["T_c2w"]), "T_w2c": torch.where(two, s2["T_w2c"], s1["T_w2c"]), "num_points": num,
            "stage": two.to(torch.int32) + 1, "idx": idx, "stage1": s1, "stage2": s2}
