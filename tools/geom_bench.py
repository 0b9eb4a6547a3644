"""Timing of the keypoint geometry (nerf_loc_amd/keypoints.py) at the shipped size: 480 x 640, stride 8, ten support views.

    python tools/geom_bench.py [--out profiles/geom_bench.jsonl] [--reps 30]

Every comparison is a drop-in on the library against the SAME module's eager formulation (keypoints.eager_*) in the same process on the same tensors, eager timed
before and after the library (tools/appearance_bench.py: compare).  JSON lines, APPENDED to --out:
  what = "piece"     select_3d_keypoints at 1024 and 100 000 points x 10 views (exact size: one read-back in both formulations) and its padded form (none in the
                     library's); build_3d_2d_pairs at 1024 and 100 000 points; conf_matrix_target at (1024, 4800) against zeros + index-put in fp32 and against
                     the reference's chain zeros().long() + index-put + .float()
  what = "estimate"  the geometry of one cascade `estimate`: select over 100 000 points x 10 views, select again with one pose, build_3d_2d_pairs twice (1024 points)
  what = "counts"    device launches (kernels and copies seen by torch.profiler) and synchronising torch calls (torch.cuda.set_sync_debug_mode) of one such
                     estimate and of each piece, per formulation; null where the profiler is not available
ms_* ("wall"): a step timed on its own by device events from an idle device after warm-up — launch latency, host work and read-backs are inside, and these steps
are bound by them; device_ms_* ("device"): the same step queued behind ~10 ms of other work, so the host is ahead and only the kernels' own time shows;
`spread_ms` is |eager before - eager after|; `faster_beyond_spread` is the README's criterion for a default.
Needs a HIP device: a timing taken elsewhere says nothing.  Run it under a time limit of its own (the whole run is well under two minutes).
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd import keypoints as kp  # noqa: E402
from tests import geom_cases as gc  # noqa: E402
from tools.appearance_bench import compare  # noqa: E402

H, W, STRIDE, F, THR, V = 480, 640, 8, 525.0, 0.05, 10
M = (H // STRIDE) * (W // STRIDE)


def count(fn):
    """(launches, synchronising torch calls) of one fn(): device events of torch.profiler, warnings of the sync debug mode."""
    fn()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
        syncs = sum("synchroniz" in str(w.message) for w in caught)
    except Exception as e:
        print("sync debug mode unavailable:", e, file=sys.stderr)
        syncs = None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:   # no tracer on this installation
        print("profiler unavailable:", e, file=sys.stderr)
        launches = None
    return launches, syncs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geom_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    case = gc.Case("bench", 0, V, H, W, STRIDE, F, THR, "scene", 9)
    K = torch.from_numpy(gc.intrinsics(case)).to(dev)
    poses = torch.from_numpy(np.stack([gc.make_pose(rng) for _ in range(V)])).to(dev)
    query = torch.from_numpy(gc.make_pose(rng, spread=0.1)).to(dev)
    query64 = query.double()   # what Matcher.localize leaves on the device
    pts = {n: torch.from_numpy(gc.sample_points(rng, n, "scene")).to(dev) for n in (1024, 100000)}
    depth = torch.from_numpy((3.0 + rng.random((H, W))).astype(np.float32)).to(dev)
    gt_j = torch.from_numpy(np.where(rng.random(1024) < 0.5, rng.integers(0, M, 1024), -1).astype(np.int32)).to(dev)
    extra = {"H": H, "W": W, "stride": STRIDE, "views": V}

    def switch(library):
        kp.PREFER_LIBRARY.update(select=library, pairs=library, target=library)

    def select(n, padded=False):
        def make(library):
            def step():
                switch(library)
                return (kp.select_3d_keypoints_padded if padded else kp.select_3d_keypoints)(pts[n], poses, K, H, W)
            return step
        return make

    def pairs(n, padded=False):
        def make(library):
            def step():
                switch(library)
                return (kp.build_3d_2d_pairs_padded if padded else kp.build_3d_2d_pairs)(pts[n], H, W, K, query, THR, STRIDE, depth_map=depth)
            return step
        return make

    def target(reference_chain=False):
        def make(library):
            def step():
                switch(library)
                if library or not reference_chain:
                    return kp.conf_matrix_target(gt_j, M)
                return kp.eager_conf_matrix_target(gt_j, M, torch.int64).float()
            return step
        return make

    def estimate(library):
        def step():
            switch(library)
            idx = kp.select_3d_keypoints(pts[100000], poses, K, H, W)
            out = kp.build_3d_2d_pairs(pts[1024], H, W, K, query, THR, STRIDE, depth_map=depth)
            idx2 = kp.select_3d_keypoints(pts[100000], query64[None], K, H, W)   # the cascade step: the pose stays on the device, in fp64
            out2 = kp.build_3d_2d_pairs(pts[1024], H, W, K, query64, THR, STRIDE, depth_map=depth)
            return idx, out, idx2, out2
        return step

    big = torch.randn((8192, 8192), device=dev)
    big_out = torch.empty_like(big)
    busy = lambda: torch.mm(big, big, out=big_out)   # ~10 ms of fp32 matmul: longer than any step's host time

    steps = [("piece", "select_3d_keypoints 1024 x 10", select(1024)), ("piece", "select_3d_keypoints 100000 x 10", select(100000)),
             ("piece", "select_3d_keypoints_padded 100000 x 10", select(100000, True)),
             ("piece", "build_3d_2d_pairs 1024", pairs(1024)), ("piece", "build_3d_2d_pairs 100000", pairs(100000)),
             ("piece", "build_3d_2d_pairs_padded 1024", pairs(1024, True)),
             ("piece", "conf_matrix_target 1024 x 4800 fp32 (eager: zeros + index-put)", target()),
             ("piece", "conf_matrix_target 1024 x 4800 fp32 (eager: the reference's zeros().long() + index-put + .float())", target(True)),
             ("estimate", "cascade estimate: 2 x select (100000), 2 x pairs (1024)", estimate)]
    lines, defaults = [], dict(kp.PREFER_LIBRARY)
    try:
        # what is timed computes the same thing (random points, no guard band: a point within an fp64 rounding of a decision could differ)
        extra["same_result_as_eager"] = bool(torch.equal(select(100000)(True)(), select(100000)(False)()) and
                                             torch.equal(pairs(100000)(True)()[3], pairs(100000)(False)()[3]) and torch.equal(target()(True)(), target(True)(False)()))
        for what, name, make in steps:
            lines += compare(what, name, make, args.reps, args.warmup, extra, busy)
        for what, name, make in steps:
            for library in (False, True):
                launches, syncs = count(make(library))
                lines.append(dict(what="counts", name=name, path="library" if library else "eager", launches=launches, synchronising_calls=syncs, **extra))
    finally:
        kp.PREFER_LIBRARY.update(defaults)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                print(json.dumps(line), flush=True)
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
