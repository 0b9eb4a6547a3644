"""Timing of the per-frame encoder (DepthFusionNet.encode): the library (libnerfloc_cnn.so, `hip_encode`) against the module's own eager path on MIOpen.

    python tools/dfnet_bench.py [--out profiles/dfnet_bench.jsonl] [--reps 20]

Without --step this is the driver: every GPU step runs as a child process under a time limit of its own (`timeout -k 10 <seconds>`), the steps are chained, and the
first one that fails ends the run.  JSON lines, APPENDED to --out:
  what = "encode"   V x H x W = 10 x 256 x 336 and 10 x 480 x 640: library against eager in the same process on the same tensor, eager timed before and after the
                    library (tools/appearance_bench.py: compare)
  what = "counts"   device launches (kernels and copies seen by torch.profiler) of one encode per path; null where the profiler is not available
  what = "setup"    the whole per-frame setup at config 2 (10 views, 256 x 336) with the switch off and on: tools/setup_bench.py's measurement (setup + first batch
                    minus a warm batch, the minimum of three)
ms_* ("wall"): a step timed on its own by device events from an idle device after warm-up — launch latency and host work are inside; device_ms_* ("device"): the
same step queued behind ~10 ms of other work, so the host is ahead and only the kernels' own time shows; `spread_ms` is |eager before - eager after|;
`faster_beyond_spread` is the README's criterion for a recommendation.
Needs a HIP device: a timing taken elsewhere says nothing.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((10, 256, 336), (10, 480, 640))
STEP_LIMIT_S = 150


def emit(out, lines):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


def module_for(seed, dev):
    from nerf_loc_amd.depth_fusion import DepthFusionNet
    from tests import dfnet_cases as dc
    m = DepthFusionNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in dc.make_weights(seed).items()}, strict=True)
    return m.to(dev).eval()


def step_encode(args):
    from tests import dfnet_cases as dc
    from tools.appearance_bench import compare
    from tools.geom_bench import count
    V, H, W = [int(s) for s in args.shape.split("x")]
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    x = torch.from_numpy(dc.make_input(V, H, W, 3)).to(dev)
    m = module_for(3, dev)
    extra = {"V": V, "H": H, "W": W}

    def make(library):
        def step():
            m.hip_encode = library
            return m.encode(x)
        return step

    big = torch.randn((8192, 8192), device=dev)
    big_out = torch.empty_like(big)
    busy = lambda: torch.mm(big, big, out=big_out)   # ~10 ms of fp32 matmul: longer than the step's host time
    a, b = make(True)().double(), make(False)().double()
    extra["library_vs_eager_rel"] = float((a - b).abs().max() / b.abs().max())
    lines = compare("encode", f"DepthFusionNet.encode {V} x {H} x {W}", make, args.reps, args.warmup, extra, busy)
    for library in (False, True):
        launches, _ = count(make(library))
        lines.append(dict(what="counts", name=f"DepthFusionNet.encode {V} x {H} x {W}", path="library" if library else "eager", launches=launches, **extra))
    emit(args.out, lines)


def step_setup(args):
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    from nerf_loc_amd.synth import CONFIGS, add_setup_inputs, make_depth_fusion_weights, make_frame, make_rays, make_weights
    cfg = CONFIGS["c2"]
    margs = NS(multires=10, multires_views=4, i_embed=0, backbone2d_fpn_dim=cfg.C, model_3d_hidden_dim=cfg.W,
               render=NS(N_samples=cfg.S, N_importance=cfg.N_importance, N_rand=1024, chunk=4096, lindisp=False, white_bkgd=False,
                         use_render_uncertainty=True, render_feature=True),
               use_scene_coord_memorization=False, matcher_hidden_dim=192, use_depth_supervision=False, matching=NS(fine_num_3d_keypoints=1024))
    frame = add_setup_inputs(cfg, make_frame(cfg))
    rays = make_rays(cfg, frame)
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    w = dict(make_weights(cfg))
    w.update(make_depth_fusion_weights(cfg.seed))
    data = {k: torch.from_numpy(frame[k]).to(dev) for k in ("topk_images", "topk_depths", "topk_Ks", "topk_poses", "feat_fine_src", "feat_coarse_src",
                                                           "depth_range", "K", "pose")}
    data.update({"embedding_a": None, "H": frame["H"], "W": frame["W"], "stride_fine": 4, "stride_coarse": 8})
    rd = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in rays.items()}
    nets = {}
    for on in (False, True):
        nets[on] = ConditionalNeRF(margs, precision="bf16x3", hip_frame_cnn=on).to(dev).eval()
        nets[on].load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)

    def measure(net):
        def first():
            net.support_neural_points = None
            net.multiview_aggregator.vis_featmaps = None
            return net.render_rays(data, rd)

        def wall(fn):
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return min(ts)
        first()
        torch.cuda.synchronize()
        t_first, t_batch = wall(first), wall(lambda: net.render_rays(data, rd))
        return 1e3 * (t_first - t_batch), 1e3 * t_first, 1e3 * t_batch

    res = {}
    for label, on in (("off_before", False), ("on", True), ("off_after", False)):
        res[label] = measure(nets[on])
    emit(args.out, [dict(what="setup", name=f"per-frame setup, config 2 ({cfg.V} views, {cfg.H} x {cfg.Wimg})", setup_ms_switch_off=res["off_before"][0],
                         setup_ms_switch_on=res["on"][0], setup_ms_switch_off_after=res["off_after"][0],
                         spread_ms=abs(res["off_before"][0] - res["off_after"][0]), first_batch_ms_off=res["off_before"][1], first_batch_ms_on=res["on"][1],
                         warm_batch_ms=res["off_before"][2])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfnet_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", choices=("encode", "setup"))
    ap.add_argument("--shape", default="10x256x336")
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit("dfnet_bench.py needs a HIP device: a timing taken elsewhere says nothing")
        return step_encode(args) if args.step == "encode" else step_setup(args)
    me = [sys.executable, os.path.abspath(__file__), "--out", args.out, "--reps", str(args.reps), "--warmup", str(args.warmup)]
    steps = [me + ["--step", "encode", "--shape", "x".join(map(str, s))] for s in SHAPES] + [me + ["--step", "setup"]]
    for cmd in steps:   # chained: the first step that fails (or runs into its limit) ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S)] + cmd).returncode
        if rc != 0:
            raise SystemExit(f"step {' '.join(cmd[-4:])} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
