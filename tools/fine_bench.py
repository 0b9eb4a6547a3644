"""Timing of the fine matcher: nl_fine_windows and nl_fine_match (through nerf_loc_amd.fine_matching) per precision against the reference's formulation in eager
PyTorch on the same device in the same process, at the shipped size: M 1024 matches, fine map 240 x 320 x 192, window stride 4, Cout = C = 192.

    python tools/fine_bench.py [--out profiles/fine_bench.jsonl] [--reps 20] [--inner 20]

Inputs are the `c192` recipe of tests/fine_cases.py scaled up (no reference import).  One JSON line per (stage, path), APPENDED to --out: median ms per call from
device events around `inner` back-to-back calls (a single call is tens of microseconds: one event pair around it would time the events), after warm-up; bytes
written, computed from the shapes; for every library line the speed-up over the eager line of the same stage and the largest difference of what the two computed.
The eager lines are timed before and after the library modes, so both see the same clocks.
Eager stage 1 is the reference's: F.unfold of the whole map, the 'n (c ww) l -> n l ww c' view, the [b_ids, j_ids] gather, Linear.  Eager stage 2: einsum, the
MLP, softmax, expectation, std.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess  # noqa: E402
from tests import fine_cases as fc  # noqa: E402


def eager_windows(pre, feat_f1, b_ids, j_ids, stride):
    u = F.unfold(feat_f1, kernel_size=(7, 7), stride=stride, padding=3)
    n, cww, l = u.shape
    u = u.view(n, cww // 49, 49, l).permute(0, 3, 2, 1)          # 'n (c ww) l -> n l ww c'
    return pre.proj(u[b_ids, j_ids])


def eager_match(fm, f0, f1, kc):
    C = f0.shape[1]
    sim = fm.mlps(torch.einsum("mc,mrc->mrc", f0, f1)).squeeze(-1)
    heat = torch.softmax((1.0 / C ** 0.5) * sim, dim=1)
    g = torch.linspace(-1, 1, 7, device=heat.device)
    grid = torch.stack([g[None, :].expand(7, 7), g[:, None].expand(7, 7)], dim=-1).reshape(1, 49, 2)
    coords = (grid * heat[:, :, None]).sum(dim=1)
    var = torch.sum(grid ** 2 * heat[:, :, None], dim=1) - coords ** 2
    std = torch.sum(torch.sqrt(torch.clamp(var, min=1e-10)), -1)
    return torch.cat([coords, std.unsqueeze(1)], -1), kc + coords * 3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--modes", default="bf16x3,fp32,bf16")
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--map", default="240x320")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fine_bench.py needs a HIP device: a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    Hf, Wf = (int(v) for v in args.map.split("x"))
    c = fc.make_case(fc.scaled("c192", args.M, Hf, Wf))
    case = c["case"]
    M, Cf, Cout, s = len(c["j_ids"]), case.Cf, case.Cout, case.s
    Ly, Lx = fc.grid_shape(Hf, Wf, s)
    feat = torch.from_numpy(c["feat_f"]).to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # as Matcher passes it: an NHWC tensor, permuted
    b_ids, j_ids = torch.from_numpy(c["b_ids"]).to(dev), torch.from_numpy(c["j_ids"]).to(dev)
    f0, kc = torch.from_numpy(c["feat_f0"]).to(dev), torch.from_numpy(c["mkps2d_c"]).to(dev)
    mods = {}
    for mode in args.modes.split(","):
        pre, fm = FinePreprocess(fc.preprocess_config(case), precision=mode), FineMatching(fc.matching_config(case), precision=mode)
        pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()})
        fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()})
        mods[mode] = (pre.to(dev).eval(), fm.to(dev).eval())
    pre0, fm0 = mods[next(iter(mods))]
    shape = {"M": M, "B": case.B, "Hf": Hf, "Wf": Wf, "Cf": Cf, "Cout": Cout, "stride": s}
    lines = []
    with torch.no_grad():
        f1 = eager_windows(pre0, feat, b_ids, j_ids, s).contiguous()
        e_ref, _ = eager_match(fm0, f0, f1, kc)
        win = {"eager": timed(lambda: eager_windows(pre0, feat, b_ids, j_ids, s), args.reps, args.inner)}
        mat = {"eager": timed(lambda: eager_match(fm0, f0, f1, kc), args.reps, args.inner)}
        diff_w, diff_m = {}, {}
        for mode, (pre, fm) in mods.items():
            win[mode] = timed(lambda pre=pre: pre.windows(feat, b_ids, j_ids, s), args.reps, args.inner)
            mat[mode] = timed(lambda fm=fm: fm.match(f0, f1, kc), args.reps, args.inner)
            diff_w[mode] = float((pre.windows(feat, b_ids, j_ids, s) - f1).abs().max())
            diff_m[mode] = float((fm.match(f0, f1, kc)[0][:, :2] - e_ref[:, :2]).abs().max())
        win["eager"] += timed(lambda: eager_windows(pre0, feat, b_ids, j_ids, s), args.reps, args.inner, 1)
        mat["eager"] += timed(lambda: eager_match(fm0, f0, f1, kc), args.reps, args.inner, 1)
    written = {
        "windows": {"lib": M * 49 * Cout * 4, "eager": (case.B * Cf * 49 * Ly * Lx + M * 49 * Cf + M * 49 * Cout) * 4},          # unfold, gather, Linear
        "match": {"lib": M * 5 * 4, "eager": (M * 49 * (Cout + 128 + 128 + 1 + 1) + M * (2 * 49 * 2 + 2 + 2 + 2 + 1 + 3 + 2)) * 4},  # x, hidden, logits, heat-map, moments
    }
    for stage, res, diff, sym in (("windows", win, diff_w, "nl_fine_windows"), ("match", mat, diff_m, "nl_fine_match")):
        med_e = float(np.median(res["eager"]))
        for path, ms in res.items():
            med = float(np.median(ms))
            line = {"stage": stage, **shape, "path": "eager" if path == "eager" else f"{sym}/{path}", "ms_median": med, "ms_min": float(np.min(ms)),
                    "ms_max": float(np.max(ms)), "timed_windows": len(ms), "calls_per_window": args.inner,
                    "bytes_written": written[stage]["eager" if path == "eager" else "lib"], "device": torch.cuda.get_device_name(0)}
            if path != "eager":
                line["speedup_vs_eager"] = med_e / med
                line["max_abs_diff_vs_eager"] = diff[path]
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
