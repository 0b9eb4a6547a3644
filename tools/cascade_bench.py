"""Two-stage cascade localisation at the shipped shape: the exact-size composition against cascade.localize_cascade, eager and replayed from a graph, in one process.

    python tools/cascade_bench.py [--out profiles/cascade_bench.jsonl] [--frames 30] [--reps 5] [--no-profile]

Shape: tools/head_bench.py's — N 1024 3-D points, coarse map 60 x 80, fine map 240 x 320, C 192, 1024 pose hypotheses, the planted scene with one camera pose.
The image bounds (H, W) of the visibility selection set how many points stage two sees: three widths, for counts near 25 %, 50 % and 90 % of N.  Paths:
  a  baseline   the parent's way: Matcher.localize, keypoints.select_3d_keypoints (a read-back), indexing, Matcher.forward (two read-backs), pose.absolute_pose,
                and the host's `if len(idx) > 0`.  Timed TWICE per repetition, before and after the new paths (a_baseline, a_baseline_again): its spread is the yardstick.
  b  cascade    cascade.localize_cascade, eager: one chain of launches, no read-back; stage two computes all N rows whatever the count
  c  graph      b captured once with torch.cuda.graph and replayed
One JSON line per (bounds, path); --out is OVERWRITTEN: `wall_ms` = host clock over `frames` cascades ending in ONE synchronise, per cascade, median / min / max over
`reps` repetitions; `issue_ms` = the host clock over the same loop before the synchronise (how long the CPU is busy per cascade; the baseline's contains its
read-backs); `launches` = device-side operations (kernels, memsets, copies) per cascade and `sync_calls` = runtime calls that wait for the device per cascade
(stream / device / event synchronise, and copies to the host), both from torch.profiler in a run of its own (null when the profiler gives no such events).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import head_bench as hb  # noqa: E402
from nerf_loc_amd import cascade, keypoints, pose  # noqa: E402
from nerf_loc_amd.position_encoding import PositionEmbeddingSine, get_embedder  # noqa: E402

BOUNDS = ((1000, 330), (1000, 650), (1000, 1150))   # (H, W) in pixels: planted cells lie 16 px apart on 1264 x 944, the unplanted points in 900 x 900


def profile_counts(fn, iters=5):
    """(device-side operations, waiting runtime calls) per call, or (None, None)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        dev = waits = 0
        for e in prof.events():
            name = e.name
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                dev += 1
            elif name.startswith("hip") and ("Synchronize" in name or name in ("hipMemcpy", "hipMemcpyWithStream", "hipMemcpyDtoH")):
                waits += 1
        waits -= 1   # the loop's own closing synchronise
        return (round(dev / iters, 1), round(max(waits, 0) / iters, 1)) if dev else (None, None)
    except Exception as exc:   # the measurement is optional; the timings stand without it
        print("profiler unavailable:", exc, file=sys.stderr)
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_bench.jsonl"))
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cascade_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lines = []
    with torch.no_grad():
        m, data = hb.build("mid", dev)
        mf, _ = hb.build("mid", dev)   # a second matcher with weights of its own in memory
        pos_fn = PositionEmbeddingSine(hb.SHIP.C // 2, normalize=True, sine_type="lin_sine")
        embed, _ = get_embedder(32, 0, include_input=False)
        data["pos_emd_3d"] = embed(data["pts3d_ndc"])
        data["pos_emd_2d"] = pos_fn(torch.zeros(1, hb.SHIP.Hc, hb.SHIP.Wc, device=dev)).reshape(-1, hb.SHIP.C)
        Kd = torch.tensor([[hb.K[0], 0, hb.K[2]], [0, hb.K[1], hb.K[3]], [0, 0, 1]], dtype=torch.float32, device=dev)
        for H, W in BOUNDS:
            def baseline():
                s1 = m.localize(data, hb.K, hb.THR, hypotheses=hb.HYP)
                idx = keypoints.select_3d_keypoints(data["kps3d"], s1["T_c2w"][None], Kd, H, W)
                if len(idx) == 0:
                    return s1["T_c2w"], 0
                sub = dict(data)
                for k in cascade.POINT_KEYS:
                    sub[k] = data[k][idx]
                d = mf(sub)
                r = pose.absolute_pose(d["mkps2d_f"] * d["stride_fine"], d["mkps3d"], hb.K, hb.THR, hypotheses=hb.HYP)
                return r["T_c2w"], len(idx)

            def eager():
                r = cascade.localize_cascade(m, mf, data, hb.K, H, W, hb.THR, hypotheses=hb.HYP)
                return r["T_c2w"], r["num_points"]
            for fn in (baseline, eager):   # warm: weights packed, tables cached
                for _ in range(3):
                    res = fn()
            torch.cuda.synchronize()
            T_base, count = baseline()
            T_new, n_new = eager()
            same = bool(torch.equal(T_base, T_new)) and int(n_new) == count
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap = eager()
            g.replay()
            torch.cuda.synchronize()
            same_graph = bool(torch.equal(cap[0], T_new))
            fns = {"a_baseline": baseline, "b_cascade": eager, "c_graph": g.replay, "a_baseline_again": baseline}
            wall, issue = {n: [] for n in fns}, {n: [] for n in fns}
            for _ in range(args.reps):
                for name, fn in fns.items():   # the paths in turn inside each repetition, the baseline first and last
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        fn()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    issue[name].append((t1 - t0) / args.frames * 1e3)
                    wall[name].append((t2 - t0) / args.frames * 1e3)
            for name, fn in fns.items():
                launches, waits = (None, None) if args.no_profile or name == "a_baseline_again" else profile_counts(fn)
                line = {"bench": "cascade", "bounds": [H, W], "path": name, "stage_two_points": count, "N": hb.SHIP.N, "coarse": [hb.SHIP.Hc, hb.SHIP.Wc], "C": hb.SHIP.C,
                        "hypotheses": hb.HYP, "frames": args.frames, "reps": args.reps, "wall_ms": round(float(np.median(wall[name])), 4),
                        "wall_ms_min": round(min(wall[name]), 4), "wall_ms_max": round(max(wall[name]), 4), "issue_ms": round(float(np.median(issue[name])), 4),
                        "launches": launches, "sync_calls": waits, "cascade_equals_baseline": same, "graph_equals_cascade": same_graph,
                        "device": torch.cuda.get_device_name(0)}
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:   # one run, one file: a second run replaces the lines
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
