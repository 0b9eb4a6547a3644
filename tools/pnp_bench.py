"""Timing of the absolute-pose solver at the shipped size: M 1024 matches (the `hard` scene of tests/pnp_cases.py: 70 % outliers, 0.5 px noise, thr 8), H 1024
hypotheses, B = 1 and B = 8 problems per call.

    python tools/pnp_bench.py [--out profiles/pnp_bench.jsonl] [--reps 20] [--inner 20]

One JSON line per (B, path), APPENDED to --out: median ms per call from device events around `inner` back-to-back calls, after warm-up.  Paths: `nl_pnp_ransac`
(the library call with its buffers allocated once) and `absolute_pose_batch` (nerf_loc_amd.pose: the call plus the allocations and the 4 x 4 transforms).  No
reference line: the reference's solver is an external CPU package that is not part of this repository's environment.  `head_eval_ms` is the sum of the matcher
head's five eval calls from the README, so that a reader sees what share of the head the pose is.
"""
import argparse
import ctypes as ct
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd import _lib, pose  # noqa: E402
from tests import pnp_cases as pc  # noqa: E402

HEAD_EVAL_MS = 3.1   # README: S2DMatching + FinePreprocess + FineMatching + both SelfCrossTransformers, eval, shipped sizes


def timed(fn, reps, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pnp_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    M, H = args.M, args.H
    lines = []
    for B in (int(b) for b in args.batches.split(",")):
        scenes = [pc.make_scene(M, 0.7, 0.5, seed=b) for b in range(B)]
        p2 = torch.from_numpy(np.concatenate([s["pts2d"] for s in scenes])).to(dev)
        p3 = torch.from_numpy(np.concatenate([s["pts3d"] for s in scenes])).to(dev)
        off = (ct.c_int32 * (B + 1))(*[b * M for b in range(B + 1)])
        intr = (ct.c_double * (4 * B))(*(list(pc.K) * B))
        thr = (ct.c_double * B)(*([8.0] * B))
        need = lib.nl_pnp_workspace_bytes(B * M, B, H)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(B, 12, dtype=torch.float64, device=dev)
        mask = torch.empty(B * M, dtype=torch.uint8, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def call():
            _lib.check(lib.nl_pnp_ransac(p2.data_ptr(), p3.data_ptr(), off, intr, thr, B, H, 0, 4, out.data_ptr(), mask.data_ptr(), info.data_ptr(), None, ws.data_ptr(),
                                         need, st), "nl_pnp_ransac")
        probs = [{"pts2d": p2[b * M:(b + 1) * M], "pts3d": p3[b * M:(b + 1) * M], "K": pc.K, "thr": 8.0} for b in range(B)]
        res = {"nl_pnp_ransac": timed(call, args.reps, args.inner), "absolute_pose_batch": timed(lambda: pose.absolute_pose_batch(probs, hypotheses=H), args.reps, args.inner)}
        torch.cuda.synchronize()
        inf = info.cpu().numpy()
        errs = [pc.pose_error(out[b].cpu().numpy(), scenes[b]["R"], scenes[b]["t"]) for b in range(B)]
        for path, ms in res.items():
            med = float(np.median(ms))
            line = {"stage": "pnp", "M": M, "H": H, "B": B, "path": path, "ms_median": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
                    "ms_per_problem": med / B, "timed_windows": len(ms), "calls_per_window": args.inner, "head_eval_ms": HEAD_EVAL_MS, "share_of_head": med / HEAD_EVAL_MS,
                    "success": int(inf[:, 0].sum()), "num_inliers": inf[:, 1].tolist(), "worst_deg": float(max(e[0] for e in errs)),
                    "worst_units": float(max(e[1] for e in errs)), "device": torch.cuda.get_device_name(0)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
