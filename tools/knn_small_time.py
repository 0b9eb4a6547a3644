"""KNN on a descriptor-sized batch (1024 support points as queries) and the time of set_frame, c2 frame."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from nerf_loc_amd.renderer import HipRenderer
from nerf_loc_amd.synth import CONFIGS, make_frame, make_weights

cfg = CONFIGS["c2"]
dev = torch.device("cuda:0")
frame = make_frame(cfg)
r = HipRenderer(cfg.W, cfg.C, cfg.S_total, "bf16x3")
r.load_weights({k: torch.from_numpy(v) for k, v in make_weights(cfg).items()})
args = [torch.as_tensor(frame[k]).to(dev) if isinstance(frame[k], np.ndarray) else frame[k] for k in ("topk_images", "feat_fine_src", "vis_featmaps")]
sup = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in frame["support_fine"].items()}
def sf():
    r.set_frame(args[0], args[1], args[2], frame["topk_Ks"], frame["topk_poses"], cfg.near, cfg.far, sup)
for _ in range(3): sf()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): sf()
torch.cuda.synchronize(); t_sf = (time.perf_counter() - t0) / 20 * 1e3
q = sup["xyz"][:1024].contiguous()
for K in (8, 1):
    for _ in range(10): r.knn(q, K)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(200): r.knn(q, K)
    e1.record(); torch.cuda.synchronize()
    print(f"knn 1024 queries K={K}: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per search")
print(f"set_frame: {t_sf:.3f} ms per call (M = {sup['xyz'].shape[0]})")
