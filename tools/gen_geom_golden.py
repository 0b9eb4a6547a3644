"""Writes tests/golden/geom_*.npz: the OUTPUTS of the reference's NerfPoseEstimator.select_3d_keypoints and .build_3d_2d_pairs on the recipes of tests/geom_cases.py.

Build container only: imports the reference's package in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE) — and calls the two
methods as unbound functions with a stub `self` (they read self.training, self.args.train_nerf and, for the per-point depth source, self.model_3d).  Modules that
nerf_pose_estimator.py imports at its top but that the two methods never call (pycolmap, ...) are stubbed in sys.modules where they are not installed; which ones
were is recorded in every file (`stubbed_modules`).  kornia is handled as in tools/gen_head_golden.py.  Nothing of the reference's program text is copied: the
files hold results and the reference's own fp32-versus-fp64 deviations.

Every recipe is run in fp32 and in fp64 and REFUSED unless (a) both runs return the same visible indices, the same valid set and the same pairs, (b) the guard
band of tests/geom_cases.py is at least 8 times the recipe's own measured |fp32 - fp64| in u, v (pixels; over the points with z >= 0.05 that project within one
image size of the frame) and z, (b') EVERY point in front of the camera is at least 8 times its own |fp32 - fp64| away from the nearest decision, and (c) no
point lies inside the band — so the tests may demand the reference's decisions on every point (`excluded_share` = 0).  The valid set is the reference's pair list at thr = inf (every valid point is
then depth-consistent).  `used_fallback` is the restatement's flag (the reference returns none); it is accepted only if the reference's pairs are the valid set
exactly when it is 1.

    python tools/gen_geom_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import geom_cases as gc  # noqa: E402
from tests import geom_ref as gr  # noqa: E402


class _Stub(types.ModuleType):
    """A module that is imported but never called: any attribute is a placeholder class."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def load_reference(ref_root):
    try:
        import kornia  # noqa: F401
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kornia_standin
        kornia_standin.install()
    sys.path.insert(0, ref_root)
    stubbed = []
    for _ in range(32):
        try:
            return importlib.import_module("nerf_loc.models.nerf_pose_estimator").NerfPoseEstimator, stubbed
        except ModuleNotFoundError as e:
            if not e.name or e.name in ("nerf_loc", "nerf_loc.models", "nerf_loc.models.nerf_pose_estimator", "nerf_loc.models.utils"):
                raise   # what the two methods do run has to be the reference's own (a checkout may lack other files, e.g. models/superpoint.py)
            sys.modules[e.name] = _Stub(e.name)
            stubbed.append(e.name)
    raise RuntimeError(f"too many missing modules: {stubbed}")


class _Model3D:
    """What the renderer branch of build_3d_2d_pairs calls: the depth of the valid points comes from the recipe's per-point array."""
    def __init__(self, depth_valid):
        self.depth_valid = depth_valid

    def points_2d_to_rays(self, uv, H, W, K, pose):
        assert len(uv) == len(self.depth_valid)
        return {}

    def render_rays(self, data, rays):
        return {"depth": self.depth_valid}


def run(Ref, case, dtype, thr):
    c = case["case"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    pts, K, query = t(case["pts"]), t(case["K"]), t(case["query"])
    self = types.SimpleNamespace(training=False, args=types.SimpleNamespace(train_nerf=False))
    vis = Ref.select_3d_keypoints(self, pts, [t(p) for p in case["poses"]], K, c.H, c.W)
    pyramid = {"conv1": torch.zeros(1, 1, 1, 1)}
    if case["depth_points"]:
        valid = gr.project(case["pts"], case["query"], case["K"], c.H, c.W)[3]   # outside the band: the reference's own valid set (checked by the caller)
        self = types.SimpleNamespace(training=True, args=types.SimpleNamespace(train_nerf=True), model_3d=_Model3D(t(case["depth"][valid])))
        out = Ref.build_3d_2d_pairs(self, None, pts, c.H, c.W, K, query, feat_pyramid_2d=pyramid, thr=thr, stride=c.stride, depth_map=None,
                                    data={"depth_range": [None]}) if valid.any() else None
        if out is None:   # no valid point: the reference would index None; the recipe list has no such case
            raise AssertionError("depth_points recipe without a valid point")
    else:
        out = Ref.build_3d_2d_pairs(self, None, pts, c.H, c.W, K, query, feat_pyramid_2d=pyramid, thr=thr, stride=c.stride, depth_map=t(case["depth"]))
    _, grid, proj, pairs = out
    return vis.numpy(), grid.numpy(), proj.numpy(), pairs.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    Ref, stubbed = load_reference(args.reference)
    print("stubbed modules:", stubbed or "none")
    torch.set_num_threads(8)
    for name in gc.GOLDEN_CASES:
        case = gc.make_case(name)
        c = case["case"]
        assert gc.excluded_share(case) == 0.0, f"{name}: points inside the band"
        v32, grid, p32, pairs32 = run(Ref, case, torch.float32, c.thr)
        v64, _, p64, pairs64 = run(Ref, case, torch.float64, c.thr)
        _, _, _, all32 = run(Ref, case, torch.float32, float("inf"))
        _, _, _, all64 = run(Ref, case, torch.float64, float("inf"))
        assert np.array_equal(v32, v64), f"{name}: fp32 and fp64 see different points: choose another seed"
        assert np.array_equal(pairs32, pairs64) and np.array_equal(all32, all64), f"{name}: fp32 and fp64 build different pairs: choose another seed"
        ref = gr.build_pairs(case["pts"], case["query"], case["K"], c.H, c.W, c.stride, c.thr, case["depth"], case["depth_points"])
        # the deviation is measured where the band has to cover it: z >= 0.05 and a projection within one image size of the frame.  Farther out |u| and with it
        # the fp32 error grow without bound, and so does the distance to a decision: those points are held to their own margin below, as every point is
        with np.errstate(all="ignore"):
            front = np.isfinite(p64).all(axis=1) & (ref["z64"] >= 0.05) & (np.abs(p64[:, 0] * c.stride - c.W / 2) <= 1.5 * c.W) & \
                (np.abs(p64[:, 1] * c.stride - c.H / 2) <= 1.5 * c.H)
        dev_uv = float(np.abs(p32[front].astype(np.float64) - p64[front]).max() * c.stride) if front.any() else 0.0
        with np.errstate(all="ignore"):   # every point in front of the camera: its distance to the nearest decision against its own deviation
            px = p64 * c.stride
            margin = np.minimum.reduce([np.abs(px[:, 0]), np.abs(px[:, 0] - c.W), np.abs(px[:, 1]), np.abs(px[:, 1] - c.H)])
            margin = np.where(ref["valid"], np.minimum(margin, np.abs(px - np.rint(px)).min(axis=1)), margin)
            dev_i = np.abs(p32.astype(np.float64) - p64).max(axis=1) * c.stride
            near = np.isfinite(px).all(axis=1) & (ref["z64"] > 0)
        assert c.kind == "edge" or (margin[near] >= 8 * dev_i[near]).all(), f"{name}: a point is nearer to a decision than 8 x its own fp32 deviation"
        z32 = (case["pts"].astype(np.float32) @ np.linalg.inv(case["query"].astype(np.float32))[:3, :3].T + np.linalg.inv(case["query"].astype(np.float32))[:3, 3])[:, 2]
        dev_z = float(np.abs(z32[front].astype(np.float64) - ref["z64"][front]).max()) if front.any() else 0.0
        if c.kind != "edge":
            assert gc.BAND_PX >= 8 * dev_uv and gc.BAND_Z >= 8 * dev_z, f"{name}: the band is less than 8 x the deviation ({dev_uv:.2e} px, {dev_z:.2e})"
        else:
            assert dev_uv == 0.0, f"{name}: the edge recipe is not exact ({dev_uv:.2e} px)"
        fallback = int(ref["info"][3])
        assert np.array_equal(pairs32, all32) if fallback else True, f"{name}: the restatement falls back, the reference's pairs are not its valid set"
        assert fallback == int(c.kind in ("fallback", "behind")), f"{name}: used_fallback = {fallback}"
        assert len(v32) == 0 if c.kind == "behind" else len(v32) > 0, f"{name}: {len(v32)} visible points"
        arrays = {"vis_idx": v32, "valid_idx": all32[0], "pairs": pairs32, "proj": p32, "proj64": p64, "grid": grid.astype(np.int32),
                  "used_fallback": np.int32(fallback), "dev_uv_px": np.float64(dev_uv), "dev_z": np.float64(dev_z),
                  "band": np.array([gc.BAND_PX, gc.BAND_Z, gc.BAND_DEPTH]), "excluded_share": np.float64(gc.excluded_share(case)),
                  "stubbed_modules": np.array(stubbed, dtype=str), "N": np.int64(c.N)}
        path = os.path.join(gc.golden_dir(), f"geom_{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 200 * 1024, f"{path} is {os.path.getsize(path)} bytes"
        print(f"{name}: N {c.N}, {len(v32)} visible, {len(all32[0])} valid, {pairs32.shape[1]} pairs, fallback {fallback}; fp32 vs fp64 {dev_uv:.2e} px, {dev_z:.2e} z; "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
