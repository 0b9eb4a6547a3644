"""Times PoseOptimizer.refine on the c2 scene (W 256, 128 samples, 10 views): the library loop (libnerfloc_refine.so around the render pair, one captured graph
per step) against the eager formulation of the same module in the same process.  Appends one JSON line per case to profiles/refine_bench.jsonl.

    python tools/refine_bench.py [--rays 512] [--steps 50] [--repeats 3] [--count-launches]

Per case (use_feat on / off, B poses x rays per pose): eager is timed before AND after the library loop (its spread is what a difference has to beat);
"wall" is one whole refine() from an idle device to a synchronised result, "issue" the host time until refine() returns (the library loop does not wait for the
device; the eager formulation reads the loss back every step, as the reference does, so its issue time is its wall time).  A batch whose kept activations do not
fit diff_render.KEEP_BYTES takes the eager formulation whatever hip_loop says: the `path` field tells.  --count-launches counts the device kernels per step of
each formulation with torch.profiler (a run of its own, 3 steps)."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from types import SimpleNamespace as NS  # noqa: E402

from nerf_loc_amd.conditional_nerf import ConditionalNeRF  # noqa: E402
from nerf_loc_amd.pose_optimizer import PoseOptimizer  # noqa: E402
from nerf_loc_amd.synth import CONFIGS, add_setup_inputs, make_depth_fusion_weights, make_frame, make_rays, make_weights  # noqa: E402


def module_and_data(cfg, dev, precision):
    args = NS(multires=10, multires_views=4, i_embed=0, backbone2d_fpn_dim=cfg.C, model_3d_hidden_dim=cfg.W,
              render=NS(N_samples=cfg.S, N_importance=cfg.N_importance, N_rand=1024, chunk=2048, lindisp=bool(cfg.lindisp), white_bkgd=False,
                        use_render_uncertainty=True, render_feature=True),
              use_scene_coord_memorization=False, matcher_hidden_dim=192, use_depth_supervision=False, matching=NS(fine_num_3d_keypoints=1024))
    frame = add_setup_inputs(cfg, make_frame(cfg))
    net = ConditionalNeRF(args, precision=precision).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in {**make_weights(cfg), **make_depth_fusion_weights(cfg.seed)}.items()}, strict=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    data = {k: t(frame[k]) for k in ("topk_images", "topk_depths", "topk_Ks", "topk_poses", "feat_fine_src", "feat_coarse_src", "depth_range", "K", "pose")}
    data.update({"embedding_a": None, "H": frame["H"], "W": frame["W"], "stride_fine": 4, "stride_coarse": 8})
    rng = np.random.default_rng(0)
    data["img"] = t(rng.random((3, cfg.H, cfg.Wimg)).astype(np.float32))
    data["feat_pyramid"] = {"layer1": t(rng.standard_normal((1, cfg.C, cfg.H // 4, cfg.Wimg // 4)).astype(np.float32))}
    return net, data, make_rays(cfg, frame)


def timed(fn, repeats):
    """[(wall s, issue s)] of `repeats` calls, each from an idle device."""
    out = []
    for _ in range(repeats):
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0, t1 - t0))
    return out, res


def launches_per_step(fn_of_steps, steps=3):
    """Device kernels per step: the difference between a run of `steps` + 1 and one of 1 step, divided by `steps` (setup kernels cancel)."""
    from torch.profiler import ProfilerActivity, profile

    def count(n):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn_of_steps(n)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return (count(steps + 1) - count(1)) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = CONFIGS[a.config]
    net, data, rays = module_and_data(cfg, dev, a.precision)
    rng = np.random.default_rng(1)
    med = lambda xs: float(np.median(xs))   # noqa: E731
    for use_feat in (True, False):
        for B, Rp in ((1, a.rays), (4, a.rays), (4, a.rays // 4)):
            uv = torch.from_numpy(rays["pixel_coordinates"][rng.choice(cfg.R, Rp, replace=False)]).to(dev)
            poses = data["pose"].double()[None].repeat(B, 1, 1)
            poses[:, :3, 3] += torch.from_numpy(rng.standard_normal((B, 3)) * 0.01).to(dev)
            opt = PoseOptimizer(net.args, net, use_feat=use_feat)
            run = lambda hip, steps=a.steps: (setattr(opt, "hip_loop", hip), opt.refine(poses, data, uv=uv, max_steps=steps, lr=1e-3, scale=None))[1]   # noqa: E731
            for hip in (False, True):   # warm both: frame tables, graph captures, allocator
                run(hip, 3)
            e1, re = timed(lambda: run(False), a.repeats)
            h, rh = timed(lambda: run(True), a.repeats)
            e2, _ = timed(lambda: run(False), a.repeats)
            ew = [w for w, _ in e1 + e2]
            row = {"tool": "refine_bench", "config": a.config, "precision": a.precision, "use_feat": use_feat, "B": B, "rays_per_pose": Rp, "steps": a.steps,
                   "path_hip_loop": rh["path"], "eager_wall_ms_before": med([w for w, _ in e1]) * 1e3, "eager_wall_ms_after": med([w for w, _ in e2]) * 1e3,
                   "eager_wall_ms_min": min(ew) * 1e3, "eager_wall_ms_max": max(ew) * 1e3, "eager_issue_ms": med([i for _, i in e1 + e2]) * 1e3,
                   "hip_wall_ms": med([w for w, _ in h]) * 1e3, "hip_wall_ms_min": min(w for w, _ in h) * 1e3, "hip_wall_ms_max": max(w for w, _ in h) * 1e3,
                   "hip_issue_ms": med([i for _, i in h]) * 1e3,
                   "hip_ms_per_step": med([w for w, _ in h]) * 1e3 / a.steps, "eager_ms_per_step": med(ew) * 1e3 / a.steps,
                   "loss_hip": [float(x) for x in rh["loss_last"].cpu()], "loss_eager": [float(x) for x in re["loss_last"].cpu()],
                   "accepted_hip": [int(x) for x in rh["accepted"].cpu()], "accepted_eager": [int(x) for x in re["accepted"].cpu()]}
            row["hip_beats_eager_beyond_spread"] = bool(row["hip_wall_ms_max"] < row["eager_wall_ms_min"])
            if a.count_launches:
                row["launches_per_step_hip"] = launches_per_step(lambda n: run(True, n))
                row["launches_per_step_eager"] = launches_per_step(lambda n: run(False, n))
            print(json.dumps(row), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
