"""Timing and accuracy of the 2-D backbone (Backbone.forward, ResNet-50 to layer2 + FPN): the library (libnerfloc_backbone.so, `hip_forward`) against the
module's own eager path on MIOpen.

    python tools/backbone_bench.py [--out profiles/backbone_bench.jsonl] [--reps 10]

Without --step this is the driver: every GPU step runs as a child process under a time limit of its own (`timeout -k 10 <seconds>`), the steps are chained, and the
first one that fails ends the run.  JSON lines, APPENDED to --out:
  what = "forward"   V x H x W = 11 x 256 x 336 and 11 x 480 x 640, fpn_dim 192: library against eager under no_grad in the same process on the same tensor, eager
                     timed before and after the library (tools/appearance_bench.py: compare); one pair of lines per precision the library has
  what = "counts"    device launches (kernels and copies seen by torch.profiler) of one forward per path, next to the header's NLB_BACKBONE_LAUNCHES
  what = "accuracy"  2 x 480 x 640 against the module's own fp64 CPU run: the library, the module in fp32 on the CPU, and eager on the GPU (MIOpen); max |err| /
                     max |ref| per output
  what = "kernels"   per-kernel times of the library's forward at 11 x 480 x 640 from one `rocprofv3 --kernel-trace --stats` run of its own (the program after
                     `--`, no counters in that run) per precision, and the achieved TFLOP/s of each convolution class against the 155 TF of
                     v_mfma_f32_32x32x2_f32 ("fp32") or a third of the 2500 TF of v_mfma_f32_32x32x16_bf16 ("bf16x3"; conv1 stays on the fp32 MFMA)
ms_* ("wall"): a step timed on its own by device events from an idle device after warm-up — launch latency and host work are inside; device_ms_* ("device"): the
same step queued behind ~10 ms of other work, so the host is ahead and only the kernels' own time shows; `spread_ms` is |eager before - eager after|;
`faster_beyond_spread` is the README's criterion for a recommendation.
Needs a HIP device: a timing taken elsewhere says nothing.
"""
import argparse
import glob
import json
import os
import re
import shutil
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((11, 256, 336), (11, 480, 640))
FPN_DIM = 192
PEAK_F32_TF = 155.0          # v_mfma_f32_32x32x2_f32
PEAK_BF16_TF = 2500.0        # v_mfma_f32_32x32x16_bf16, dense; three MFMAs per product in "bf16x3": a third of it is the yardstick
STEP_LIMIT_S = 300
TRACE_CALLS = 6


def emit(out, lines):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


def module_for(seed, dev, dtype=torch.float32):
    from nerf_loc_amd.backbone2d import Backbone
    from tests import backbone_cases as bc
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=FPN_DIM)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in bc.make_weights(seed, FPN_DIM).items()}, strict=True)
    return m.to(device=dev, dtype=dtype).eval()


def library_precisions():
    """The precisions this build of the library runs (a refused one is left out and named)."""
    from nerf_loc_amd import _backbone_lib
    from tests import backbone_cases as bc
    dev = torch.device("cuda:0")
    w = bc.make_weights(1, 64)
    packed = _backbone_lib.pack_weights([torch.from_numpy(w[n]).to(dev) for n in _backbone_lib.weight_names()], 64)
    have = []
    for p in _backbone_lib.PRECISIONS:
        try:
            _backbone_lib.backbone_forward(packed, torch.rand(1, 3, 16, 16, device=dev), 64, precision=p)
            have.append(p)
        except RuntimeError:
            pass
    return have


def conv_gflop(V, H, W, F):
    """{class: GFLOP} of one forward (2 flop per multiply-add), by the convolution kernel's class."""
    from tests.backbone_cases import plane_sizes
    (h1, w1), (h2, w2), (h3, w3) = plane_sizes(H, W)
    n1, n2, n3 = V * h1 * w1, V * h2 * w2, V * h3 * w3
    g = {"7x7": 2.0 * n1 * 147 * 64, "1x1": 0.0, "3x3": 0.0}
    inpl = 64
    for b in range(3):
        g["1x1"] += 2.0 * n2 * (inpl * 64 + 64 * 256 + (inpl * 256 if b == 0 else 0))
        g["3x3"] += 2.0 * n2 * 64 * 64 * 9
        inpl = 256
    for b in range(4):
        nin = n2 if b == 0 else n3
        g["1x1"] += 2.0 * (nin * inpl * 128 + n3 * 128 * 512 + (n3 * inpl * 512 if b == 0 else 0))
        g["3x3"] += 2.0 * n3 * 128 * 128 * 9
        inpl = 512
    g["1x1"] += 2.0 * (n3 * 512 * F + n2 * 256 * F)
    g["3x3"] += 2.0 * (n3 + n2) * F * F * 9
    return {k: v / 1e9 for k, v in g.items()}


def step_forward(args):
    from nerf_loc_amd import _backbone_lib
    from tests import backbone_cases as bc
    from tools.appearance_bench import compare
    from tools.geom_bench import count
    V, H, W = [int(s) for s in args.shape.split("x")]
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    x = torch.from_numpy(bc.make_images(V, H, W, 3)).to(dev)
    m = module_for(3, dev)
    big = torch.randn((8192, 8192), device=dev)
    big_out = torch.empty_like(big)
    busy = lambda: torch.mm(big, big, out=big_out)   # ~10 ms of fp32 matmul: longer than the step's host time
    lines = []
    have = library_precisions()
    for precision in _backbone_lib.PRECISIONS:
        extra = {"V": V, "H": H, "W": W, "fpn_dim": FPN_DIM, "precision": precision, "gflop": sum(conv_gflop(V, H, W, FPN_DIM).values())}
        if precision not in have:
            lines.append(dict(what="forward", name=f"Backbone.forward {V} x {H} x {W}", path="library", status="NL_ERR_UNSUPPORTED in this build", **extra))
            continue

        def make(library):
            def step():
                m.hip_forward, m.hip_precision = library, precision
                return m(x)
            return step
        a, b = make(True)(), make(False)()
        extra["library_vs_eager_rel"] = {k: float((a[k].double() - b[k].double()).abs().max() / b[k].double().abs().max()) for k in a}
        lines += compare("forward", f"Backbone.forward {V} x {H} x {W}", make, args.reps, args.warmup, extra, busy)
        for library in ((False, True) if precision == have[0] else (True,)):
            launches, _ = count(make(library))
            lines.append(dict(what="counts", name=f"Backbone.forward {V} x {H} x {W}", path="library" if library else "eager", launches=launches,
                              header_launches=_backbone_lib.LAUNCHES if library else None, **extra))
    emit(args.out, lines)


def step_accuracy(args):
    from tests import backbone_cases as bc
    V, H, W = 2, 480, 640
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.set_num_threads(16)
    imgs = torch.from_numpy(bc.make_images(V, H, W, 4))
    want = {k: v.numpy() for k, v in module_for(4, "cpu", torch.float64)(imgs.double()).items()}
    rel = lambda got, k: float(np.abs(got.double().cpu().numpy() - want[k]).max() / np.abs(want[k]).max())
    lines = [dict(what="accuracy", name=f"{V} x {H} x {W}", path="fp32 on the CPU", err={k: rel(v, k) for k, v in module_for(4, "cpu")(imgs).items()})]
    m = module_for(4, dev)
    x = imgs.to(dev)
    lines.append(dict(what="accuracy", name=f"{V} x {H} x {W}", path="eager on the GPU (MIOpen)", err={k: rel(v, k) for k, v in m(x).items()}))
    m.hip_forward = True
    for precision in library_precisions():
        m.hip_precision = precision
        lines.append(dict(what="accuracy", name=f"{V} x {H} x {W}", path=f"library {precision}", err={k: rel(v, k) for k, v in m(x).items()}))
    emit(args.out, lines)


def step_traced(args):
    """The program rocprofv3 runs: TRACE_CALLS library forwards and nothing else worth a kernel."""
    from tests import backbone_cases as bc
    V, H, W = [int(s) for s in args.shape.split("x")]
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    m = module_for(3, dev)
    m.hip_forward, m.hip_precision = True, args.precision
    x = torch.from_numpy(bc.make_images(V, H, W, 3)).to(dev)
    for _ in range(TRACE_CALLS):
        m(x)
    torch.cuda.synchronize()


def step_kernels(args):
    V, H, W = [int(s) for s in args.shape.split("x")]
    name = f"Backbone.forward {V} x {H} x {W}"
    if not shutil.which("rocprofv3"):
        return emit(args.out, [dict(what="kernels", name=name, status="rocprofv3 not found")])
    tmp = tempfile.mkdtemp(prefix="backbone_kt_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "rocpd", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--step", "traced",
           "--shape", args.shape, "--precision", args.precision]
    res = subprocess.run(cmd, capture_output=True, text=True)
    dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
    if res.returncode != 0 or not dbs:
        return emit(args.out, [dict(what="kernels", name=name, status=f"rocprofv3 ended with {res.returncode}", stderr=res.stderr[-400:])])
    db = sqlite3.connect(dbs[0])
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    scol = [r[1] for r in db.execute(f"pragma table_info({ks})")]
    name_col = "display_name" if "display_name" in scol else ("kernel_name" if "kernel_name" in scol else "name")
    rows = list(db.execute(f"select s.{name_col}, count(*), sum(d.end-d.start) from {kd} d join {ks} s on d.kernel_id = s.id group by s.{name_col} order by 3 desc"))
    rows = [(re.sub(r"\s+", " ", n), c, t) for n, c, t in rows if "bb_" in n and "bb_pack" not in n and "bb_fold" not in n]   # the one-time packing is left out
    per_call = {n: dict(launches_per_forward=c / TRACE_CALLS, ms_per_forward=t / 1e6 / TRACE_CALLS) for n, c, t in rows}
    gflop = conv_gflop(V, H, W, FPN_DIM)
    classes = {}
    for cls, ks_ in (("7x7", "7"), ("1x1", "1"), ("3x3", "3")):
        ms = sum(v["ms_per_forward"] for n, v in per_call.items() if re.search(r"bb_conv3?_kernel<\s*%s\s*," % ks_, n))
        peak = PEAK_BF16_TF / 3 if args.precision == "bf16x3" and cls != "7x7" else PEAK_F32_TF
        classes[cls] = dict(gflop=gflop[cls], ms=ms, tflops=gflop[cls] / ms if ms else None, peak_tf=peak, share_of_peak=gflop[cls] / ms / peak if ms else None)
    shutil.rmtree(tmp, ignore_errors=True)
    emit(args.out, [dict(what="kernels", name=name, precision=args.precision, forwards=TRACE_CALLS, total_ms_per_forward=sum(v["ms_per_forward"] for v in per_call.values()),
                         launches_per_forward=sum(v["launches_per_forward"] for v in per_call.values()), classes=classes, kernels=per_call)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", choices=("forward", "accuracy", "kernels", "traced"))
    ap.add_argument("--shape", default="11x256x336")
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit("backbone_bench.py needs a HIP device: a timing taken elsewhere says nothing")
        return {"forward": step_forward, "accuracy": step_accuracy, "kernels": step_kernels, "traced": step_traced}[args.step](args)
    me = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--reps", str(args.reps), "--warmup", str(args.warmup)]
    steps = [me + ["--step", "forward", "--shape", "x".join(map(str, s))] for s in SHAPES] + [me + ["--step", "accuracy"]]
    steps += [me + ["--step", "kernels", "--shape", "x".join(map(str, SHAPES[-1])), "--precision", p] for p in ("fp32", "bf16x3")]
    for cmd in steps:   # chained: the first step that fails (or runs into its limit) ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd).returncode
        if rc != 0:
            raise SystemExit(f"step {' '.join(cmd[-4:])} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
