"""Timing of SelfCrossTransformer: nl_sct_forward (through nerf_loc_amd.transformer) per precision against the module's own eager path (eval mode, no_grad:
nn.MultiheadAttention with need_weights=False, so torch may take its fused attention) on the same device in the same process, at the two shipped shapes:
coarse B 1, N0 1024, N1 4800, C 192, F 512 and fine B 1024, N0 1, N1 49, C 192, F 128.

    python tools/sct_bench.py [--out profiles/sct_bench.jsonl] [--reps 20]

Inputs and weights are the recipe of tests/sct_cases.py at those shapes (gain 8; no reference import).  One JSON line per (shape, path), APPENDED to --out: median ms
per call from device events around 10 back-to-back calls (a call is about a millisecond: one event pair around it would time the events too), after warm-up; the algorithmic
FLOP count (projections, both attention products, out_proj, FFN: 2 per multiply-add, no padding, no split terms) and the rate it gives; the bytes the library writes
(q, k, v, the attention output and the layer output of every layer), computed from the shapes; for the eager line the bytes the reference's formulation writes for
the per-head scores and probabilities alone (computed, not measured: torch's fused attention may write less).  The eager line is timed before and after the library
modes, so both see the same clocks.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd.transformer import SelfCrossTransformer  # noqa: E402
from tests import sct_cases as sc  # noqa: E402

SHAPES = {"coarse": sc.SctCase("coarse", 192, 512, 1, 1024, 4800, 8.0, 61), "fine": sc.SctCase("fine", 192, 128, 1024, 1, 49, 8.0, 62)}
INNER = {"coarse": 10, "fine": 10}


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


def counts(case):
    """(algorithmic FLOP, bytes the library writes, bytes of the per-head scores + probabilities of the reference's formulation) of one forward."""
    B, C, Fh = case.B, case.C, case.F
    flop = lib = scores = 0
    for nq, nk in ((case.N0, case.N0), (case.N1, case.N1), (case.N0, case.N1), (case.N1, case.N0)):
        flop += B * (2 * C * C * (nq + 2 * nk) + 4 * nq * nk * C + 2 * nq * C * C + 4 * nq * C * Fh)
        lib += B * ((nq + 2 * nk) + 2 * nq) * C * 4
        scores += B * 2 * sc.NHEAD * nq * nk * 4
    return flop, lib, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sct_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    ap.add_argument("--shapes", default="coarse,fine")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sct_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        c = sc.make_case(case)
        ins = [torch.from_numpy(c[k]).to(dev) for k in ("v0", "pos0", "v1", "pos1")]
        mods = {}
        for mode in args.modes.split(","):
            m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, precision=mode)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()})
            mods[mode] = m.to(dev).eval()
        m0 = mods[next(iter(mods))]
        inner = INNER[shape]
        flop, lib_bytes, score_bytes = counts(case)
        with torch.no_grad():
            ref = m0._eager(*ins)
            scale = [float(r.abs().max()) for r in ref]
            res = {"eager": timed(lambda: m0._eager(*ins), args.reps, inner)}
            diff = {}
            for mode, m in mods.items():
                res[mode] = timed(lambda m=m: m(*ins), args.reps, inner)
                out = m(*ins)
                diff[mode] = max(float((o - r).abs().max()) / s for o, r, s in zip(out, ref, scale))
            res["eager"] += timed(lambda: m0._eager(*ins), args.reps, inner, 1)
        med_e = float(np.median(res["eager"]))
        for path, ms in res.items():
            med = float(np.median(ms))
            line = {"shape": shape, "B": case.B, "N0": case.N0, "N1": case.N1, "C": case.C, "F": case.F, "path": "eager" if path == "eager" else f"nl_sct_forward/{path}",
                    "ms_median": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "timed_windows": len(ms), "calls_per_window": inner,
                    "algorithmic_gflop": flop / 1e9, "algorithmic_tflops": flop / med / 1e9, "device": torch.cuda.get_device_name(0)}
            if path == "eager":
                line["bytes_scores_and_probabilities_if_materialised"] = score_bytes
            else:
                line["bytes_written"] = lib_bytes
                line["speedup_vs_eager"] = med_e / med
                line["max_rel_diff_vs_eager"] = diff[path]
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
