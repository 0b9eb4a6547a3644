"""Timing of the coarse matcher: the library call (nl_s2d_match through S2DMatching.match) per precision against the reference's formulation in eager
PyTorch on the same device in the same process (row-chunked so that it fits), at (N, M, C) = (1024, 4800, 192) and (1024, 9600, 192).

    python tools/match_bench.py [--out profiles/s2d_bench.jsonl] [--reps 30] [--chunk 64]

One JSON line per (size, path): median ms per call from device events (each call timed on its own, after warm-up), TFLOP/s on the 41 088-MAC-per-pair count
(2 FLOP per MAC; C x 128 + 128 x 128 + 128), the fraction of the bf16 MFMA peak bench.py uses, bytes written, and for every library line the speed-up over
the eager line of the same size.  The eager path alternates with the library modes inside one timed session so that both see the same clocks.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd.matching import S2DMatching, select_mutual_nearest  # noqa: E402
from tests import match_cases as mc  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # bench.py's figure
SIZES = ((1024, 4800, 192), (1024, 9600, 192))


def macs_per_pair(C):
    return C * 128 + 128 * 128 + 128


def eager_forward(m, d0, d1, chunk):
    """The reference's eval forward (einsum -> mlps -> sigmoid -> mutual nearest), rows of desc0 in chunks."""
    rows = []
    for a in range(0, d0.shape[0], chunk):
        rows.append(m.mlps(torch.einsum("nc,mc->nmc", d0[a:a + chunk], d1)).squeeze(-1))
    score = torch.sigmoid(torch.cat(rows, dim=0))
    i_ids, j_ids = select_mutual_nearest(score, m.thr)
    return score, i_ids, j_ids


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2d_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64, help="rows of desc0 per chunk of the eager path (64 x 4800 x 192 fp32 = 236 MB for x)")
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    lines = []
    for (N, M, C) in SIZES:
        case = mc.MatchCase("bench", N, M, C, 16, 0.35, 0.2, False)
        c = mc.make_case(case)
        d0, d1 = torch.from_numpy(c["desc0"]).to(dev), torch.from_numpy(c["desc1"]).to(dev)
        mods = {}
        for mode in args.modes.split(","):
            m = S2DMatching(C, thr=c["thr"], precision=mode)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()})
            mods[mode] = m.to(dev).eval()
        ref = mods[next(iter(mods))]
        flop = 2.0 * macs_per_pair(C) * N * M
        with torch.no_grad():
            res = {"eager": timed(lambda: eager_forward(ref, d0, d1, args.chunk), args.reps, 2)}
            for mode, m in mods.items():
                res[mode] = timed(lambda m=m: m.match(d0, d1), args.reps, args.warmup)
            res["eager"] += timed(lambda: eager_forward(ref, d0, d1, args.chunk), args.reps, 1)   # again after the library modes: same session, both ends
            # what was timed computes the same thing
            s_e, i_e, j_e = eager_forward(ref, d0, d1, args.chunk)
            agree = {}
            for mode, m in mods.items():
                s, mj, _ = m.match(d0, d1)
                agree[mode] = float((s - s_e).abs().max())
        med_e = float(np.median(res["eager"]))
        for path, ms in res.items():
            med = float(np.median(ms))
            line = {"N": N, "M": M, "C": C, "path": path if path == "eager" else f"nl_s2d_match/{path}", "ms_median": med, "ms_min": float(np.min(ms)),
                    "ms_max": float(np.max(ms)), "timed_calls": len(ms), "tflops": flop / (med * 1e-3) / 1e12,
                    "frac_bf16_peak": flop / (med * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, "bytes_written": N * M * 4 + 2 * N * 4 + (N + M) * 4}
            if path == "eager":
                line["chunk_rows"] = args.chunk
                line["bytes_written"] = int(N * M * (C + 128 + 128 + 1 + 1) * 4)   # x, two hidden tensors, logits, scores
            else:
                line["speedup_vs_eager"] = med_e / med
                line["max_abs_score_diff_vs_eager"] = agree[path]
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
