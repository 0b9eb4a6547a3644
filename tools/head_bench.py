"""Descriptors in, pose out: per-frame time of the localisation head at the shipped shape, four ways, in one process.

    python tools/head_bench.py [--out profiles/head_bench.jsonl] [--frames 50] [--reps 5] [--no-kernel-time]

Shape: N 1024 3-D points, coarse map 60 x 80 (4800 cells), fine map 240 x 320, C 192, 1024 pose hypotheses; the recipe is tests/head_cases.py's with planted
partners (three quarters of the points), so several hundred rows match.  Per frame the inputs are the descriptors, the maps, pts3d_ndc and the key points;
BOTH position encodings (the coarse map's sine table, the embedder of pts3d_ndc) are part of the frame, as they are in the reference's estimator.  Paths:
  a  composition   what a user of the five drop-in modules writes: the eager position encodings (PositionEmbeddingSine._eager on the coarse map and on the M fine
                   windows, the eager embedder), the module calls, the glue of the reference's Matcher.forward, pose.absolute_pose.  The baseline.
  b  forward       Matcher.forward (library encodings, cached tables) + pose.absolute_pose: exact shapes, two host read-backs
  c  localize      Matcher.localize: padded to N rows, the count on the device, no read-back
  d  graph         c captured once with torch.cuda.graph and replayed
One JSON line per (scene, path), APPENDED to --out: `wall_ms` = host clock over `frames` frames ending in ONE synchronise, per frame, the median and the spread over
`reps` repetitions, the paths taken in turn inside each repetition; `issue_ms` = the host clock over the same loop before the synchronise (how long the CPU is
busy per frame; for a and b it contains the two read-backs); `kernel_ms` = the sum of the device's kernel durations per frame from torch.profiler, in a run of its
own.  Scenes: `mid` (the recipe), `low` (all but 128 points lose their partner; many of them still find a mutual-nearest cell above the threshold, so the count
stays in the hundreds) and `high` (every point planted) for c and d against a and b; every line carries its match count.
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
from nerf_loc_amd import pose  # noqa: E402
from nerf_loc_amd.matcher import Matcher  # noqa: E402
from nerf_loc_amd.position_encoding import PositionEmbeddingSine, get_embedder  # noqa: E402
from tests import head_cases as hc  # noqa: E402
from tests import pnp_cases as pc  # noqa: E402

SHIP = hc.HeadCase("ship", 192, 1024, 60, 80, 240, 320, 81, 0.05)
K = (500.0, 500.0, 640.0, 480.0)
THR, HYP = 24.0, 1024   # a planted pair is off by at most 3 fine cells x stride_fine = 12 px per axis


def build(scene, dev):
    c = hc.make_case(SHIP)
    d = c["data"]
    rng = np.random.default_rng(1)
    partner = c["planted"].copy()
    if scene == "low":     # rows 128.. get fresh descriptors: their planted partner no longer resembles them
        d["desc_3d"][128:] = rng.standard_normal(d["desc_3d"][128:].shape).astype(np.float32)
        partner[128:] = -1
    elif scene == "high":  # the last quarter gets partners too, among the cells nobody was planted on
        free = np.setdiff1d(np.arange(len(d["desc_2d_coarse"])), partner[partner >= 0])
        rows = np.nonzero(partner < 0)[0]
        partner[rows] = free[:len(rows)]
        d["desc_2d_coarse"][partner[rows]] = d["desc_3d"][rows] + np.float32(SHIP.noise) * rng.standard_normal((len(rows), SHIP.C)).astype(np.float32)
    # one camera pose explains every planted pair: the 3-D point of row i projects onto its partner's cell (pixels = kps2d x stride_fine), so the solver has a pose
    # to find and does its full work
    R, t = pc.rodrigues(0.3 * rng.normal(size=3)), np.array([0.1, -0.2, 0.3])
    px = rng.uniform(0, 900, size=(SHIP.N, 2))
    ok = partner >= 0
    px[ok] = d["kps2d"][partner[ok]] * hc.STRIDE_FINE
    depth = rng.uniform(2.0, 8.0, size=SHIP.N)
    cam = np.stack([(px[:, 0] - K[2]) / K[0] * depth, (px[:, 1] - K[3]) / K[1] * depth, depth], axis=1)
    d["kps3d"] = ((cam - t) @ R).astype(np.float32)
    m = Matcher(hc.Args, SHIP.C, SHIP.C, SHIP.C)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    m = m.to(dev).eval()
    data = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    for k in ("pos_emd_3d", "pos_emd_2d", "conf_matrix_gt", "pairs_gt", "kps3d_proj_gt"):
        del data[k]   # the encodings are computed per frame; the rest is for training
    data["pts3d_ndc"] = torch.from_numpy(rng.uniform(-1, 1, (SHIP.N, 3)).astype(np.float32)).to(dev)
    return m, data


def paths(m, data):
    pos_fn = PositionEmbeddingSine(SHIP.C // 2, normalize=True, sine_type="lin_sine")
    embed, _ = get_embedder(32, 0, include_input=False)
    coarse_map = torch.zeros(1, SHIP.Hc, SHIP.Wc, device=data["desc_3d"].device)
    W = m.fine_window_size

    def compose():
        d = dict(data)
        d["pos_emd_3d"] = embed.eager(d["pts3d_ndc"])
        d["pos_emd_2d"] = pos_fn._eager(coarse_map).reshape(-1, SHIP.C)
        a, b = m.coarse_transformer(d["desc_3d"][None], d["pos_emd_3d"][None], d["desc_2d_coarse"][None], d["pos_emd_2d"][None])
        d = m.coarse_matcher(a[0], b[0], d)
        i_ids, j_ids = d["i_ids"], d["j_ids"]
        d["b_ids"] = torch.zeros_like(i_ids)
        d.update({"mkps3d": d["kps3d"][i_ids], "mkps2d_c": d["kps2d"][j_ids]})
        M = len(i_ids)
        f3, p3 = d["desc_3d_fine"][i_ids][:, None, :], d["pos_emd_3d"][i_ids][:, None, :]
        win = m.fine_preprocess(d["feat_fine"].permute(0, 3, 1, 2), None, d)
        pw = pos_fn._eager(win[..., 0].view(M, W, W)).view(M, W * W, -1)
        f3, win = m.fine_transformer(f3, p3, win, pw)
        d = m.fine_matcher(f3[:, 0, :], win, d)
        return pose.absolute_pose(d["mkps2d_f"] * d["stride_fine"], d["mkps3d"], K, THR, hypotheses=HYP), M

    def encodings(d):
        d["pos_emd_3d"] = embed(d["pts3d_ndc"])
        d["pos_emd_2d"] = pos_fn(coarse_map).reshape(-1, SHIP.C)
        return d

    def forward():
        d = m(encodings(dict(data)))
        return pose.absolute_pose(d["mkps2d_f"] * d["stride_fine"], d["mkps3d"], K, THR, hypotheses=HYP), len(d["i_ids"])

    def localize():
        r = m.localize(encodings(dict(data)), K, THR, hypotheses=HYP)
        return r, r["num_matches"]
    return {"a_composition": compose, "b_forward": forward, "c_localize": localize}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_bench.jsonl"))
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="mid,low,high")
    ap.add_argument("--no-kernel-time", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lines = []
    with torch.no_grad():
        for scene in args.scenes.split(","):
            m, data = build(scene, dev)
            fns = paths(m, data)
            results = {}
            for name, fn in fns.items():   # warm: weights packed, tables cached, workspaces sized
                for _ in range(3):
                    results[name] = fn()
            torch.cuda.synchronize()
            matches = int(results["b_forward"][1])
            assert int(results["c_localize"][1]) == matches   # (a) may differ by a pair: its eager encodings differ from the tables in the last bit
            same = all(torch.equal(results["c_localize"][0][k], results["b_forward"][0][k]) for k in ("T_w2c", "num_inliers", "success"))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap, _ = fns["c_localize"]()
            g.replay()
            torch.cuda.synchronize()
            same_graph = all(torch.equal(cap[k], results["c_localize"][0][k]) for k in ("T_w2c", "num_inliers", "success", "num_matches"))
            fns["d_graph"] = g.replay
            wall = {n: [] for n in fns}
            issue = {n: [] for n in fns}
            for _ in range(args.reps):
                for name, fn in fns.items():   # the paths in turn inside each repetition
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        fn()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    issue[name].append((t1 - t0) / args.frames * 1e3)
                    wall[name].append((t2 - t0) / args.frames * 1e3)
            kernel = {n: None for n in fns}
            if not args.no_kernel_time:
                from torch.profiler import ProfilerActivity, profile
                for name, fn in fns.items():
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        for _ in range(10):
                            fn()
                        torch.cuda.synchronize()
                    us = sum(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0) for e in prof.key_averages())
                    kernel[name] = us / 10 / 1e3
            for name in fns:
                line = {"bench": "head", "scene": scene, "path": name, "matches": matches, "matches_composition": int(results["a_composition"][1]), "N": SHIP.N, "coarse": [SHIP.Hc, SHIP.Wc], "fine": [SHIP.Hf, SHIP.Wf],
                        "C": SHIP.C, "hypotheses": HYP, "frames": args.frames, "reps": args.reps, "wall_ms": round(float(np.median(wall[name])), 4),
                        "wall_ms_min": round(min(wall[name]), 4), "wall_ms_max": round(max(wall[name]), 4), "issue_ms": round(float(np.median(issue[name])), 4),
                        "kernel_ms": None if kernel[name] is None else round(kernel[name], 4), "success": int(results["b_forward"][0]["success"]),
                        "localize_equals_forward": bool(same), "graph_equals_localize": bool(same_graph), "device": torch.cuda.get_device_name(0)}
                lines.append(line)
                print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
