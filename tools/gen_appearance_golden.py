"""Writes tests/golden/app_*.npz: the OUTPUTS of the reference's AppearanceEmbedding and AppearanceAdaptLayer on the recipes of tests/appearance_cases.py.

Build container only: imports the reference's package in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE).  The reference's
models/appearance_embedding.py imports torchvision and its COTR backbone at module level without using either in these two classes; where torchvision is not
installed, empty stand-in modules (torchvision, torchvision.transforms, torchvision.models, torchvision.models._utils with an IntermediateLayerGetter attribute)
are registered before the import, and which was used is recorded in every file (`torchvision_source`).  Nothing of the reference's program text is copied: the files
hold results, state-dict names and shapes, and the reference's own fp32-versus-fp64 deviation per tensor (max |fp32 - fp64| / max |fp64|).

Per statistics case: the (B, 2 c) embedding in fp64.  Per adapt case: y, the MLP's code (a | b) and the fp64 autograd gradients of sum(g_y * y) with respect to x,
embedding, target_embedding, the six parameters and the code, with the recipe's g_y.  A recipe is REFUSED unless
  (a) for clip cases no fp64 y (before the clamp) lies within 1e-5 of 0 or of 1, and both sides of the mask occur, and
  (b) no fp64 pre-activation of the two LeakyReLUs lies within 1e-5 of 0
so that the tests may hold masks exactly.

    python tools/gen_appearance_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import appearance_cases as ac  # noqa: E402


def install_torchvision_standin():
    try:
        import torchvision
        return "torchvision " + getattr(torchvision, "__version__", "?")
    except ImportError:
        pass
    tv, tr, mo, ut = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.models", "torchvision.models._utils"))
    ut.IntermediateLayerGetter = type("IntermediateLayerGetter", (), {})
    tv.transforms, tv.models, mo._utils = tr, mo, ut
    for m in (tv, tr, mo, ut):
        sys.modules[m.__name__] = m
    return "stand-in (empty modules: the two classes use nothing of it)"


def load_reference(ref_root):
    source = install_torchvision_standin()
    sys.path.insert(0, ref_root)
    from nerf_loc.models import appearance_embedding
    return appearance_embedding, source


def rel(a32, a64):
    a64 = np.asarray(a64, dtype=np.float64)
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max() / max(np.abs(a64).max(), 1e-300))


def save(path, **arrays):
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"


def run_stats(ref, c, dtype):
    conv1 = torch.from_numpy(c["conv1"]).to(dtype)
    if c["case"].channels_last:
        conv1 = conv1.contiguous(memory_format=torch.channels_last)
    mod = ref.AppearanceEmbedding(ac.Args(2 * c["case"].c))
    with torch.no_grad():
        return mod(None, {"conv1": conv1}).numpy()


def run_adapt(ref, c, dtype):
    """-> y, code, the two pre-activations, the gradients of sum(g_y * y), the module's state dict"""
    case = c["case"]
    mod = ref.AppearanceAdaptLayer(ac.Args(), case.C, is_rgb=case.is_rgb)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    mod = mod.to(dtype)
    kept = {}
    mod.mlp[0].register_forward_hook(lambda m, i, o: kept.__setitem__("z1", o.detach().clone()))   # before the in-place LeakyReLU
    mod.mlp[2].register_forward_hook(lambda m, i, o: kept.__setitem__("z2", o.detach().clone()))

    def keep_code(m, i, o):
        kept["code"] = o.detach().clone()
        o.register_hook(lambda g: kept.__setitem__("g_code", g.detach().clone()))
    mod.mlp[4].register_forward_hook(keep_code)
    ins = {k: torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in ("x", "embedding", "target_embedding")}
    y = mod(ins["x"], ins["embedding"], ins["target_embedding"])
    (torch.from_numpy(c["g_y"]).to(dtype) * y).sum().backward()
    grads = {k: v.grad.numpy() for k, v in ins.items()}
    grads.update({k: p.grad.numpy() for k, p in mod.named_parameters()})
    grads["code"] = kept["g_code"].numpy()
    return y.detach().numpy(), kept["code"].numpy(), kept["z1"].numpy(), kept["z2"].numpy(), grads, mod.state_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref, source = load_reference(args.reference)
    print("torchvision:", source)
    torch.set_num_threads(8)
    gdir = ac.golden_dir()

    for name in ac.STATS_CASES:
        c = ac.make_stats_case(name)
        o32, o64 = run_stats(ref, c, torch.float32), run_stats(ref, c, torch.float64)
        n = c["case"].c
        assert o64.shape == (c["case"].B, 2 * n) and o64.dtype == np.float64
        arrays = {"out": o64, "dev_mean": np.float64(rel(o32[:, :n], o64[:, :n])), "dev_std": np.float64(rel(o32[:, n:], o64[:, n:])),
                  "torchvision_source": np.array(source)}
        print(f"stats {name}: reference fp32 vs fp64: mean {arrays['dev_mean']:.2e}, std {arrays['dev_std']:.2e}")
        save(os.path.join(gdir, f"app_stats_{name}.npz"), **arrays)

    for name in ac.ADAPT_CASES:
        c = ac.make_adapt_case(name)
        case = c["case"]
        y32, code32, _, _, _, _ = run_adapt(ref, c, torch.float32)
        y64, code64, z1, z2, g64, sd = run_adapt(ref, c, torch.float64)
        act = min(np.abs(z1).min(), np.abs(z2).min())
        assert act > ac.SAFE_MARGIN, f"{name}: a LeakyReLU pre-activation at {act:.2e}: choose another seed"
        clipped = 0.0
        if case.is_rgb:
            C = case.C
            y0 = code64[:, None, None, :C] * c["x"].astype(np.float64) + code64[:, None, None, C:]
            edge = min(np.abs(y0).min(), np.abs(y0 - 1.0).min())
            assert edge > ac.SAFE_MARGIN, f"{name}: a value {edge:.2e} from a clip boundary: choose another seed"
            clipped = float(((y0 < 0) | (y0 > 1)).mean())
            assert 0.02 < clipped < 0.98, f"{name}: {clipped:.0%} clipped: both sides of the mask must occur"
        assert list(sd.keys()) == list(ac.PARAM_NAMES)
        arrays = {"y": y64, "code": code64, "dev_y": np.float64(rel(y32, y64)), "dev_code": np.float64(rel(code32, code64)), "clipped": np.float64(clipped),
                  "state_dict_names": np.array(list(sd.keys())), "state_dict_shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64),
                  "torchvision_source": np.array(source)}
        for k in ac.GRAD_NAMES + ("code",):
            arrays["grad_" + k] = g64[k]
        print(f"adapt {name}: reference fp32 vs fp64: y {arrays['dev_y']:.2e}, code {arrays['dev_code']:.2e}; clipped {clipped:.0%}; |a| max {np.abs(code64[:, :case.C]).max():.2f}, "
              f"|b| max {np.abs(code64[:, case.C:]).max():.2f}; nearest pre-activation {act:.2e}")
        save(os.path.join(gdir, f"app_adapt_{name}.npz"), **arrays)


if __name__ == "__main__":
    main()
