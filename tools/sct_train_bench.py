"""Timing and peak memory of a SelfCrossTransformer training step at the two shipped shapes — coarse (B 1, N0 1024, N1 4800, C 192, F 512) and fine (B 1024, N0 1,
N1 49, C 192, F 128): forward + backward through the module with dropout = 0 in training mode, the library's step (hip_training = True: nl_sct_forward_train /
nl_sct_backward) per precision against the module's own eager path (hip_training = False) on the same device in the same process, the eager path timed before and
after the library modes.

    python tools/sct_train_bench.py [--out profiles/sct_train_bench.jsonl] [--reps 10] [--shapes coarse,fine] [--dropout P]

--dropout P (0 < P < 1; the default 0 is everything above, unchanged): the same step with dropout = P in training mode — the library's step with dropout inside the
kernels (hip_training and hip_dropout: nl_sct_forward_train_dropout / nl_sct_backward_dropout, path nl_sct_train_dropout/<mode>) against the module's eager path with
the same dropout (torch's masks; timed before and after, as above) and against the library's own dropout = 0 step (path nl_sct_train/<mode>), which gives the cost
of the generator (`dropout_over_no_dropout`).  Every line carries "dropout": P, and the lines are APPENDED to --out.  The masks of the two paths differ, so no
gradient is compared here (tests/test_gpu_sct_dropout.py does that with the library's masks on both sides).

One JSON line per shape and path: median / min / max ms of a step from device events (each step timed on its own, after warm-up), the peak of
torch.cuda.max_memory_allocated above the level before the step, the state and backward workspace in bytes, and for every library line the ratio to the eager
median, the spread between the two eager sessions, and the largest relative difference of the gradient at v0 from eager's.  Inputs and weights are the recipe of
tests/sct_cases.py (gain 8) at the shape; the loss is sum(g_out0 * out0) + sum(g_out1 * out1) with the seeded cotangents of tests/sct_train_cases.py.
Run it under a time limit of its own (a step is milliseconds to tens of milliseconds; the whole run a few minutes).
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
from nerf_loc_amd.transformer import SelfCrossTransformer  # noqa: E402
from tests import sct_cases as sc  # noqa: E402
from tests import sct_train_cases as stc  # noqa: E402
from tools.match_train_bench import peak_of, timed  # noqa: E402

SHAPES = {"coarse": sc.SctCase("coarse", 192, 512, 1, 1024, 4800, 8.0, 61), "fine": sc.SctCase("fine1024", 192, 128, 1024, 1, 49, 8.0, 62)}


def make_step(m, c, dev):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [t(c[k]) for k in ("v0", "pos0", "v1", "pos1")]
    g0, g1 = t(c["g_out0"]), t(c["g_out1"])

    def step():
        m.zero_grad(set_to_none=True)
        a = [x.detach().requires_grad_(i == 0) for i, x in enumerate(ins)]
        o0, o1 = m(*a)
        loss = (o0 * g0).sum() + (o1 * g1).sum()
        loss.backward()
        return loss.detach(), a[0].grad
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sct_train_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="coarse,fine")
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    ap.add_argument("--dropout", type=float, default=0.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sct_train_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        c = sc.make_case(case)
        c["g_out0"], c["g_out1"] = stc.cotangents(case)

        def module(mode, hip, dropout=0.0):
            m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, dropout=dropout, precision=mode)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()})
            m.hip_training = hip
            m.hip_dropout = hip and dropout > 0
            return m.to(dev).train()
        eager = make_step(module("bf16x3", False, args.dropout), c, dev)
        steps = {mode: make_step(module(mode, True), c, dev) for mode in args.modes.split(",")}
        if args.dropout > 0:
            steps.update({f"drop/{mode}": make_step(module(mode, True, args.dropout), c, dev) for mode in args.modes.split(",")})
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
        dims = (case.B, case.N0, case.N1, case.C, case.F)
        state_b, ws_b = int(lib.nl_sct_train_state_bytes(*dims)), int(lib.nl_sct_backward_workspace_bytes(*dims))
        med_e = float(np.median(res["eager"]))
        for path, ms in res.items():
            med = float(np.median(ms))
            name = "eager" if path == "eager" else f"nl_sct_train_dropout/{path[5:]}" if path.startswith("drop/") else f"nl_sct_train/{path}"
            line = {"shape": shape, "B": case.B, "N0": case.N0, "N1": case.N1, "C": case.C, "F": case.F, "path": name, "ms_median": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "timed_steps": len(ms), "peak_bytes": peaks[path]}
            if path == "eager":
                line.update(ms_median_before=first, ms_median_after=second, spread_ms=abs(first - second))
            elif args.dropout > 0:
                line.update(eager_over_library=med_e / med, state_bytes=state_b, backward_workspace_bytes=ws_b,
                            eager_peak_over_library_peak=peaks["eager"] / max(peaks[path], 1))
                if path.startswith("drop/"):
                    line.update(dropout_over_no_dropout=med / float(np.median(res[path[5:]])))
            else:
                loss, g = steps[path]()
                line.update(eager_over_library=med_e / med, state_bytes=state_b, backward_workspace_bytes=ws_b,
                            eager_peak_over_library_peak=peaks["eager"] / max(peaks[path], 1),
                            loss_rel_diff_vs_eager=float(((loss - loss_e).abs() / loss_e.abs()).item()),
                            g_v0_max_rel_diff_vs_eager=float(((g - g_e).abs().max() / g_e.abs().max()).item()))
            if args.dropout > 0:
                line["dropout"] = args.dropout
            lines.append(line)
            print(json.dumps(line), flush=True)
        del eager, steps
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.dropout > 0 else "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
