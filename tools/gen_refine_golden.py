"""Writes tests/golden/refine_se3.npz: the OUTPUTS of the reference's se3_exp_map / se3_log_map (nerf_loc/utils/transform/se3.py) on a handful of cases.

Needs a checkout of the reference — pass it with --reference (default: $NERFLOC_REFERENCE) — whose utils/transform package it loads in place, unmodified.  Only
that directory is loaded (se3.py, so3.py, math.py), under a package shell, so none of the reference's other modules run; models/pose_optimizer.py is NOT imported
(it needs a SuperPoint module that does not exist).  Nothing of the reference's program text is copied: the file holds results.

Per exponential case (zero rotation; angle 0.005, below the clamp; exactly 0.01; 0.3; 3.0; a 50-unit translation): the 6-vector, exp in fp64, the autograd gradient
of sum(G * exp(p)) for a fixed G, the logarithm of that matrix, exp(log(.)) of it (the reference's own round trip; `roundtrip_exact` names the cases where that gives the matrix back), and the reference's fp32-against-fp64 deviation.
For the logarithm additionally the identity.  A case on which the reference's fp32 run is off by more than 1e-4 of the fp64 value is refused.

    python tools/gen_refine_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSE = 1e-4

# name: (log-translation, rotation axis (normalised below), angle)
CASES = {
    "zero_rotation": ((0.3, -0.2, 0.5), (1.0, 0.0, 0.0), 0.0),
    "below_clamp": ((0.1, 0.4, -0.3), (0.6, -0.64, 0.48), 0.005),
    "at_clamp": ((-0.2, 0.1, 0.7), (0.0, 1.0, 0.0), 0.01),        # one axis: the squared norm is one product, whatever the summation order
    "angle_0p3": ((0.5, -1.0, 0.25), (0.36, 0.48, -0.8), 0.3),
    "angle_3p0": ((1.5, 0.5, -2.0), (-0.48, 0.6, 0.64), 3.0),
    "far_translation": ((50.0, -20.0, 35.0), (0.8, 0.0, -0.6), 0.4),
}
BELOW_CLAMP = ("zero_rotation", "below_clamp")


def load_reference(path):
    d = os.path.join(path, "nerf_loc", "utils", "transform")
    if not os.path.exists(os.path.join(d, "se3.py")):
        raise SystemExit(f"{d}/se3.py not found: pass --reference")
    pkg = types.ModuleType("_ref_transform")
    pkg.__path__ = [d]
    sys.modules["_ref_transform"] = pkg
    return importlib.import_module("_ref_transform.se3")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(np.asarray(b, np.float64)).max(), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "refine_se3.npz"))
    a = ap.parse_args()
    se3 = load_reference(a.reference)
    rng = np.random.default_rng(7)
    out = {"names": np.array(list(CASES)), "below_clamp": np.array(BELOW_CLAMP)}
    for name, (u, axis, angle) in CASES.items():
        axis = np.asarray(axis, np.float64)
        p = np.concatenate([np.asarray(u, np.float64), axis / np.linalg.norm(axis) * angle])
        G = rng.standard_normal((4, 4))
        p64 = torch.tensor(p[None], dtype=torch.float64, requires_grad=True)
        T64 = se3.se3_exp_map(p64)
        (T64 * torch.from_numpy(G)[None]).sum().backward()
        T32 = se3.se3_exp_map(torch.tensor(p[None], dtype=torch.float32))
        with torch.no_grad():
            L64 = se3.se3_log_map(T64.detach())
            L32 = se3.se3_log_map(T64.detach().float())
            RT = se3.se3_exp_map(L64)
        dev_exp, dev_log = rel(T32.numpy(), T64.detach().numpy()), rel(L32.numpy(), L64.numpy())
        if max(dev_exp, dev_log) > REFUSE:
            raise SystemExit(f"{name}: the reference's fp32 run is off by {dev_exp:.2e} (exp) / {dev_log:.2e} (log) of its fp64 value: refused")
        out.update({f"{name}.p": p, f"{name}.G": G, f"{name}.T": T64.detach().numpy()[0], f"{name}.grad": p64.grad.numpy()[0], f"{name}.log": L64.numpy()[0],
                    f"{name}.roundtrip": RT.numpy()[0], f"{name}.dev_exp32": dev_exp, f"{name}.dev_log32": dev_log})
        print(f"{name:16s} fp32 vs fp64: exp {dev_exp:.2e} log {dev_log:.2e}")
    eye = torch.eye(4, dtype=torch.float64)[None]
    with torch.no_grad():
        L = se3.se3_log_map(eye)
        L32 = se3.se3_log_map(eye.float())
        out.update({"identity.T": eye.numpy()[0], "identity.log": L.numpy()[0], "identity.roundtrip": se3.se3_exp_map(L).numpy()[0],
                    "identity.dev_log32": float(np.abs(L32.numpy() - L.numpy()).max())})
    # the cases whose matrix the reference's own exp(log(.)) gives back (the others sit at or below one of the two clamps: squared angle 1e-4, cosine 1 - 1e-4)
    out["roundtrip_exact"] = np.array([n for n in CASES if rel(out[f"{n}.roundtrip"], out[f"{n}.T"]) <= 1e-10])
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
