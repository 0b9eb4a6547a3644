"""Timing and peak memory of the fine matcher's training step at the shipped size (M 1024, fine map 240 x 320 x 192, Cout = C = 192): forward + backward through
FinePreprocess and FineMatching in training mode, the library's step (hip_training = True: nl_fine_windows / nl_fine_match and their backward calls) per
precision against the eager formulation (hip_training = False) on the same device in the same process, the eager path timed before and after the library modes.

    python tools/fine_train_bench.py [--out profiles/fine_train_bench.jsonl] [--reps 20] [--size 1024,240,320]

One JSON line per path: median / min / max ms of a step from device events (each step timed on its own, after warm-up), the peak of
torch.cuda.max_memory_allocated above the level before the step, the two backward workspaces in bytes, and for every library line the ratio to the eager median
and the spread between the two eager sessions.  The map is an NHWC tensor seen as NCHW (what a channels-last backbone hands over); the loss is l2_with_std.
Run it under a time limit of its own (a step is milliseconds; the whole run well under two minutes).
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
from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess  # noqa: E402
from tests import fine_cases as fc  # noqa: E402
from tools.match_train_bench import peak_of, timed  # noqa: E402


def make_step(pre, fm, c, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nhwc = t(c["feat_f"].transpose(0, 2, 3, 1))
    f0 = t(c["feat_f0"])
    fixed = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": t(c["b_ids"]), "j_ids": t(c["j_ids"]), "mkps2d_c": t(c["mkps2d_c"]),
             "expec_f_gt": t(c["expec_f_gt"])}

    def step():
        pre.zero_grad(set_to_none=True), fm.zero_grad(set_to_none=True)
        base, a = nhwc.detach().requires_grad_(True), f0.detach().requires_grad_(True)
        data = dict(fixed)
        fm(a, pre(base.permute(0, 3, 1, 2), None, data), data)
        data["fine_loss"].backward()
        return data["fine_loss"].detach(), base.grad
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_train_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1024,240,320")
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fine_train_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    M, Hf, Wf = (int(v) for v in args.size.split(","))
    case = fc.scaled("c192", M, Hf, Wf)
    c = fc.make_case(case)

    def modules(mode, hip):
        pre = FinePreprocess(fc.preprocess_config(case), precision=mode)
        pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()})
        fm = FineMatching(fc.matching_config(case), precision=mode)
        fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()})
        pre.hip_training = fm.hip_training = hip
        return pre.to(dev).train(), fm.to(dev).train()
    eager = make_step(*modules("bf16x3", False), c, dev)
    steps = {mode: make_step(*modules(mode, True), c, dev) for mode in args.modes.split(",")}
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
    lib = _lib.load()
    ws_match = int(lib.nl_fine_match_backward_workspace_bytes(M, case.Cout))
    ws_win = int(lib.nl_fine_windows_backward_workspace_bytes(case.Cf, case.Cout, case.B, Hf, Wf, case.s, M))
    med_e = float(np.median(res["eager"]))
    lines = []
    for path, ms in res.items():
        med = float(np.median(ms))
        line = {"M": M, "Hf": Hf, "Wf": Wf, "Cf": case.Cf, "C": case.Cout, "stride": case.s, "path": "eager" if path == "eager" else f"nl_fine_train/{path}",
                "ms_median": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "timed_steps": len(ms), "peak_bytes": peaks[path],
                "product_tensor_bytes": M * 49 * case.Cout * 4}
        if path == "eager":
            line.update(ms_median_before=first, ms_median_after=second, spread_ms=abs(first - second))
        else:
            loss, g = steps[path]()
            line.update(eager_over_library=med_e / med, match_workspace_bytes=ws_match, windows_workspace_bytes=ws_win,
                        eager_peak_over_library_peak=peaks["eager"] / max(peaks[path], 1),
                        loss_rel_diff_vs_eager=float(((loss - loss_e).abs() / loss_e.abs()).item()),
                        g_map_max_rel_diff_vs_eager=float(((g - g_e).abs().max() / g_e.abs().max()).item()))
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
