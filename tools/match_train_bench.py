"""Timing and peak memory of the coarse matcher's training step at (N, M, C) = (1024, 4800, 192): the library pair (nl_s2d_forward_train +
nl_s2d_backward_train through S2DMatching in training mode) per precision against the eager training formulation (hip_training = False: einsum -> mlps under
autograd in 32-row chunks, focal loss, backward) on the same device in the same process, the eager path timed before and after the library modes.

    python tools/match_train_bench.py [--out profiles/s2d_train_bench.jsonl] [--reps 20] [--size 1024,4800,192]

One JSON line per path: median / min / max ms of a forward + backward from device events (each step timed on its own, after warm-up), the peak of
torch.cuda.max_memory_allocated above the level before the step, the backward workspace in bytes, and for every library line the ratio to the eager median and
the spread between the two eager sessions.  Run it under a time limit of its own (a step is tens of milliseconds; the whole run well under two minutes).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd import _lib  # noqa: E402
from nerf_loc_amd.matching import S2DMatching  # noqa: E402
from tests import match_cases as mc  # noqa: E402


def make_step(m, d0, d1, gt):
    def step():
        m.zero_grad(set_to_none=True)
        a, b = d0.detach().requires_grad_(True), d1.detach().requires_grad_(True)
        data = m(a, b, {"conf_matrix_gt": gt})
        data["coarse_loss"].backward()
        return data["coarse_loss"].detach(), a.grad
    return step


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - start)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2d_train_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1024,4800,192")
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_train_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    N, M, C = (int(v) for v in args.size.split(","))
    c = mc.make_case(mc.MatchCase("bench", N, M, C, 16, 0.35, 0.2, False))
    d0, d1, gt = (torch.from_numpy(c[k]).to(dev) for k in ("desc0", "desc1", "conf_matrix_gt"))

    def module(mode, hip):
        m = S2DMatching(C, thr=c["thr"], precision=mode, eager_chunk_rows=32)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()})
        m.hip_training = hip
        return m.to(dev).train()
    eager = make_step(module("bf16x3", False), d0, d1, gt)
    steps = {mode: make_step(module(mode, True), d0, d1, gt) for mode in args.modes.split(",")}
    res = {"eager": timed(eager, args.reps, 2)}
    first = float(np.median(res["eager"]))
    for mode, st in steps.items():
        res[mode] = timed(st, args.reps, args.warmup)
    again = timed(eager, args.reps, 1)   # again after the library modes: same session, both ends
    second = float(np.median(again))
    res["eager"] += again
    peaks = {"eager": peak_of(eager)}
    peaks.update({mode: peak_of(st) for mode, st in steps.items()})
    loss_e, g_e = eager()
    ws_bytes = int(_lib.load().nl_s2d_backward_train_workspace_bytes(N, M, C))
    med_e = float(np.median(res["eager"]))
    lines = []
    for path, ms in res.items():
        med = float(np.median(ms))
        line = {"N": N, "M": M, "C": C, "path": "eager/chunk32" if path == "eager" else f"nl_s2d_train/{path}", "ms_median": med, "ms_min": float(np.min(ms)),
                "ms_max": float(np.max(ms)), "timed_steps": len(ms), "peak_bytes": peaks[path], "product_tensor_bytes": N * M * C * 4}
        if path == "eager":
            line.update(ms_median_before=first, ms_median_after=second, spread_ms=abs(first - second))
        else:
            loss, g = steps[path]()
            line.update(eager_over_library=med_e / med, workspace_bytes=ws_bytes, eager_peak_over_library_peak=peaks["eager"] / max(peaks[path], 1),
                        loss_rel_diff_vs_eager=float(((loss - loss_e).abs() / loss_e.abs()).item()),
                        g_desc0_max_rel_diff_vs_eager=float(((g - g_e).abs().max() / g_e.abs().max()).item()))
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
