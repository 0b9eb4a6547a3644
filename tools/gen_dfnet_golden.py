#!/usr/bin/env python3
"""Generate tests/golden/dfnet_*.npz by running the REFERENCE implementation's DepthFusionNet (build container only).

The reference's conditional_nerf/depth_fusion.py is imported unmodified; its one absent import (inplace_abn.ABN, unused) is stubbed as in tools/gen_golden.py.
For every recipe of tests/dfnet_cases.py the reference's `fuse_net` (with forward hooks on layer1..3), `depth_skip` and `conv_out` run on the CPU in fp64 and
again in fp32.  Written per case: out, x1, x2, x3 in fp64, and `fp32_dev_<tensor>` = max |fp32 - fp64| / max |fp64|, the reference's own fp32 error, from
which the GPU tests take their bar.  Only outputs are written; the inputs are regenerated from the recipe.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import dfnet_cases  # noqa: E402


def reference_class():
    ia = types.ModuleType("inplace_abn")
    ia.ABN = object
    sys.modules["inplace_abn"] = ia
    return importlib.import_module("nerf_loc.models.conditional_nerf.depth_fusion").DepthFusionNet


def run(cls, x, weights, dtype):
    net = cls().to(dtype).eval()
    missing = net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in weights.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    got = {}
    hooks = [getattr(net.fuse_net, f"layer{i}").register_forward_hook(lambda m, a, o, i=i: got.__setitem__(f"x{i}", o.detach().clone())) for i in (1, 2, 3)]
    with torch.no_grad():
        t = torch.from_numpy(x).to(dtype)
        feats = net.fuse_net(t)
        got["out"] = net.conv_out(torch.cat([net.depth_skip(t[:, 3:4]), feats], 1))
    for h in hooks:
        h.remove()
    return {k: v.double().numpy() for k, v in got.items()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    cls = reference_class()
    os.makedirs(os.path.join(ROOT, "tests", "golden"), exist_ok=True)
    for name in dfnet_cases.CASES:
        x, weights = dfnet_cases.build(name)
        r64, r32 = run(cls, x, weights, torch.float64), run(cls, x, weights, torch.float32)
        save = {}
        for k in dfnet_cases.TENSORS:
            save[k] = r64[k]
            save["fp32_dev_" + k] = np.float64(np.abs(r32[k] - r64[k]).max() / max(np.abs(r64[k]).max(), 1e-30))
        path = os.path.join(ROOT, "tests", "golden", f"dfnet_{name}.npz")
        np.savez_compressed(path, **save)
        print(name, x.shape, {k: float(save["fp32_dev_" + k]) for k in dfnet_cases.TENSORS}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
