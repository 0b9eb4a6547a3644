"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, f"{name}.npz")))


def rel_err(a, b):
    """max |a-b| / max(|b|)  — the 'max-rel to max' metric of SURVEY.md App. B."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / den)


def l2_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def oracle_inputs(case):
    """numpy recipe dict -> torch CPU tensors in the layout oracle.render_oracle expects."""
    from oracle.render_oracle import to_torch
    frame = to_torch(case["frame"])
    rays = to_torch(case["rays"])
    params = {k: torch.from_numpy(v) for k, v in case["weights"].items()}
    return params, frame, rays


def knn_bruteforce(points, K: int = 8, chunk: int = 4096):
    """Exact KNN by chunked distance matrices (tests only: the stand-in for `HipRenderer.knn` where no GPU is present).
    Ties: lower index first (knn_cpu.cpp:39-52 sorts (dist, idx) pairs).  -> callable q (N, 3) -> idx (N, K) int64"""
    import torch

    def f(q):
        out = []
        for i in range(0, q.shape[0], chunk):
            d = ((q[i:i + chunk, None, :] - points[None]) ** 2).sum(-1)
            out.append(torch.argsort(d, dim=1, stable=True)[:, :K])
        return torch.cat(out, 0)
    return f


# ----------------------------------------------------------------------------- scenes with surfaces (density-head rungs, nerf_loc_amd.synth.SURFACE_RUNGS)
OUT_KEYS = ("rgb", "depth", "weights", "depth_uncertainty", "feat")


def oracle_render(case, weights=None, white_bkgd=None, intermediates=False, threads=16):
    """oracle.render_oracle.render_rays on a recipe dict (cfg, frame, rays, weights[, u]); `weights` replaces the case's own."""
    from oracle import render_oracle as orc
    cfg = case["cfg"]
    params = {k: torch.from_numpy(v) for k, v in (weights or case["weights"]).items()}
    torch.set_num_threads(threads)
    with torch.no_grad():
        return orc.render_rays(params, orc.to_torch(case["frame"]), orc.to_torch(case["rays"]), cfg.S, white_bkgd=white_bkgd,
                               knn_threads=threads, intermediates=intermediates)


def density_pre_activation(weights, geo):
    """sigma_mlp.0 . geo + b (N,) for a numpy weights dict and the oracle's `geo` (N, W)."""
    import torch.nn.functional as F
    return F.linear(geo, torch.from_numpy(weights["sigma_mlp.0.weight"]), torch.from_numpy(weights["sigma_mlp.0.bias"])).reshape(-1)


def surface_weights(case, rung, thin=None):
    """The case's weights with the density head of rung `rung`, calibrated on the ORACLE's pre-activation of this scene (`thin` = the oracle's
    render of the unscaled case with intermediates, computed here when not handed in).  -> (weights, g, c)"""
    from nerf_loc_amd.synth import surface_gain_offset, with_density_head
    pre = None
    if rung != "A":
        thin = thin if thin is not None else oracle_render(case, intermediates=True)
        pre = density_pre_activation(case["weights"], thin["geo"]).numpy()
    g, c = surface_gain_offset(rung, pre)
    return with_density_head(case["weights"], g, c), g, c


def fp64_render(case, weights=None, white_bkgd=False):
    """The same function in double on the CPU (nerf_loc_amd.diff_render's eager restatement, exact KNN by distance matrices) -> dict of fp64 tensors."""
    from nerf_loc_amd import diff_render as dr
    from oracle.render_oracle import sample_depths
    cfg, frame, rays = case["cfg"], case["frame"], case["rays"]
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    p = {k: t(v) for k, v in (weights or case["weights"]).items()}
    fr = {k: t(frame[k]) for k in ("topk_Ks", "topk_poses", "topk_images", "feat_fine_src", "vis_featmaps")}
    fr.update(near=float(cfg.near), far=float(cfg.far), support={k: t(v) for k, v in frame["support_fine"].items()})
    near, far = torch.from_numpy(rays["depth_range"])
    z = sample_depths(cfg.S, near, far, cfg.lindisp).expand(cfg.R, cfg.S).contiguous().double()   # the oracle's fp32 depths, as constants
    with torch.no_grad():
        return dr.render_rays_diff(p, fr, t(rays["rays_o"]), t(rays["rays_d"]), z, t(frame["pose"]), knn_bruteforce(fr["support"]["xyz"]), white_bkgd=white_bkgd)


def first_opaque(weights, eps=1e-4):
    """Per ray: the index of the first sample whose transmittance (exclusive product of 1 - alpha = 1 - the weights before it) is below eps; S where none is."""
    w = torch.as_tensor(weights).double()
    T = 1.0 - (torch.cumsum(w, 1) - w)
    below = T < eps
    S = w.shape[1]
    return torch.where(below.any(1), below.double().argmax(1), torch.full((w.shape[0],), S))
