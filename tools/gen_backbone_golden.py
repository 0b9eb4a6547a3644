#!/usr/bin/env python3
"""Writes tests/golden/backbone_*.npz: the OUTPUTS of the reference's 2-D backbone on the recipes of tests/backbone_cases.py.

Build container only: imports the reference's models/COTR/backbone2d.py (with its resnet.py and fpn.py) in place, unmodified — pass its checkout with
--reference (default: $NERFLOC_REFERENCE).  That file imports two names from torchvision (transforms.Normalize, models._utils.IntermediateLayerGetter).  The real
torchvision is used where it is installed; otherwise tools/torchvision_standin.py, written from torchvision's documented behaviour, is registered in its place.
Which of the two produced a file is recorded in it (`torchvision_source`).

For every recipe the reference's Backbone(['conv1', 'layer1', 'layer2'], use_fpn=True, fpn_dim) runs on the CPU in fp64 and again in fp32 (forward hooks on
body.layer1 / body.layer2 take the two maps in front of the pyramid).  Written per case: conv1, layer1, layer2 (and the taps, for the smaller cases) in fp64;
`fp32_dev_<tensor>` = max |fp32 - fp64| / max |fp64| for all five, the reference's own fp32 error; the reference's state-dict key list and shapes.  A recipe on
which any of the five has fp32_dev above 1.25e-5 is REFUSED: the tests hold every tensor of every recipe to 1e-4 with no relaxed bar, so an ill-conditioned recipe
must not become a fixture.  Only results are written; weights and images are regenerated from the recipe.  Nothing of the reference's program text is copied.

    python tools/gen_backbone_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import backbone_cases as bc  # noqa: E402

GUARD = 1.25e-5


def load_reference(ref_root):
    try:
        import torchvision
        source = "torchvision " + getattr(torchvision, "__version__", "?")
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import torchvision_standin
        torchvision_standin.install()
        source = "stand-in (tools/torchvision_standin.py)"
    sys.path.insert(0, ref_root)
    return importlib.import_module("nerf_loc.models.COTR.backbone2d"), source


def run(mod, imgs, weights, fpn_dim, dtype):
    with contextlib.redirect_stdout(io.StringIO()):   # the constructor prints every frozen parameter's name
        net = mod.Backbone(return_layers=list(bc.RETURN_LAYERS), train_backbone=True, use_fpn=True, fpn_dim=fpn_dim)
    net = net.to(dtype).eval()
    res = net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in weights.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    got = {}
    hooks = [getattr(net.body, l).register_forward_hook(lambda m, a, o, l=l: got.__setitem__("tap_" + l, o.detach().clone())) for l in ("layer1", "layer2")]
    with torch.no_grad():
        got.update({k: v.detach().clone() for k, v in net(torch.from_numpy(imgs).to(dtype)).items()})
    for h in hooks:
        h.remove()
    sd = net.state_dict()
    return {k: v.double().numpy() for k, v in got.items()}, list(sd.keys()), [tuple(v.shape) for v in sd.values()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set NERFLOC_REFERENCE")
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    mod, source = load_reference(args.reference)
    out = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out, exist_ok=True)
    for name in bc.CASES:
        imgs, weights, fpn_dim = bc.build(name)
        r64, keys, shapes = run(mod, imgs, weights, fpn_dim, torch.float64)
        r32, _, _ = run(mod, imgs, weights, fpn_dim, torch.float32)
        assert [(k, tuple(s)) for k, s in zip(keys, shapes)] == bc.weight_shapes(fpn_dim), "the recipe's name list is not the reference's state dict"
        devs = {k: float(np.abs(r32[k] - r64[k]).max() / max(np.abs(r64[k]).max(), 1e-30)) for k in bc.TENSORS}
        if max(devs.values()) > GUARD:
            raise SystemExit(f"{name}: refused, the reference's own fp32 run misses its fp64 run by {devs} (above {GUARD})")
        save = {"torchvision_source": np.array(source), "state_dict_keys": np.array(keys),
                "state_dict_shapes": np.array([list(s) + [0] * (4 - len(s)) for s in shapes], dtype=np.int64)}
        save.update({"fp32_dev_" + k: np.float64(v) for k, v in devs.items()})
        save.update({k: r64[k] for k in bc.tensors_of(name)})
        for old in bc.golden_paths(ROOT, name):
            if os.path.exists(old):
                os.remove(old)
        sizes = []
        for i, part in enumerate(bc.split_for_files(save)):
            path = os.path.join(out, f"backbone_{name}.npz" if i == 0 else f"backbone_{name}.{i}.npz")
            np.savez_compressed(path, **part)
            sizes.append(os.path.getsize(path))
            assert sizes[-1] < (1 << 20), path
        print(name, imgs.shape, fpn_dim, {k: "%.3g" % v for k, v in devs.items()}, sizes, "bytes")


if __name__ == "__main__":
    main()
