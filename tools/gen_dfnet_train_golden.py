#!/usr/bin/env python3
"""Generate tests/golden/dfnet_grad_<recipe>_partN.npz by running the REFERENCE implementation's DepthFusionNet forward and backward (build container only).

The reference's conditional_nerf/depth_fusion.py is imported unmodified, with the `inplace_abn` stub of tools/gen_dfnet_golden.py.  For the recipes
tests/dfnet_train_cases.RECIPES of tests/dfnet_cases.py it runs on the CPU in fp64 and again in fp32; the loss is sum(out * cot) with the seeded cotangent of
tests/dfnet_train_cases.py.  Written per tensor: `grad_<name>`, the fp64 gradient rounded to fp32, and `fp32_dev_<name>` = max |fp32 - fp64| / max |fp64|, the
reference's own fp32 error, from which the tests take their bar; and `lo_<name>` (int16) with `lo_scale_<name>`: what the rounding to fp32 dropped, so that
grad + lo * lo_scale is the fp64 gradient to 2^-40 of its largest value and the CPU test can hold the in-repo module's fp64 autograd to it at 1e-10.  The four conv biases in front of an InstanceNorm have an identically zero gradient (autograd
leaves rounding noise there): they are recorded as zeros with fp32_dev 0, not divided.  A recipe is split into parts of at most PART_BYTES of gradient.
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

from tests import dfnet_cases, dfnet_train_cases as tc  # noqa: E402


def reference_class():
    ia = types.ModuleType("inplace_abn")
    ia.ABN = object
    sys.modules["inplace_abn"] = ia
    return importlib.import_module("nerf_loc.models.conditional_nerf.depth_fusion").DepthFusionNet


def run(cls, x, weights, cot, dtype):
    net = cls().to(dtype)
    missing = net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in weights.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    t = torch.from_numpy(x).to(dtype)
    out = net.conv_out(torch.cat([net.depth_skip(t[:, 3:4]), net.fuse_net(t)], 1))
    (out * torch.from_numpy(cot).to(dtype)).sum().backward()
    return {k: p.grad.double().numpy() for k, p in net.named_parameters()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    cls = reference_class()
    for name in tc.RECIPES:
        x, weights = dfnet_cases.build(name)
        V, H, W = dfnet_cases.CASES[name][:3]
        cot = tc.cotangent(V, H, W)
        g64, g32 = run(cls, x, weights, cot, torch.float64), run(cls, x, weights, cot, torch.float32)
        assert set(g64) == set(weights) and len(g64) == 72   # in the state dict's order
        parts, cur, size, worst = [], {}, 0, (0.0, "")
        for k in g64:
            if k in tc.ZERO_BIASES:
                print(name, k, "identically zero; autograd left", float(np.abs(g64[k]).max()), "(fp64)", float(np.abs(g32[k]).max()), "(fp32)")
                grad, dev = np.zeros(g64[k].shape, np.float32), 0.0
            else:
                grad, dev = g64[k].astype(np.float32), float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max())
            worst = max(worst, (dev, k))
            if cur and size + grad.nbytes + grad.size * 2 > tc.PART_BYTES:
                parts.append(cur)
                cur, size = {}, 0
            res = (0.0 if k in tc.ZERO_BIASES else g64[k]) - grad.astype(np.float64)
            scale = max(float(np.abs(res).max()), 1e-300) / 32767.0
            cur["grad_" + k], cur["fp32_dev_" + k] = grad, np.float64(dev)
            cur["lo_" + k], cur["lo_scale_" + k] = np.rint(res / scale).astype(np.int16), np.float64(scale)
            size += grad.nbytes + grad.size * 2
        parts.append(cur)
        for i, part in enumerate(parts, 1):
            path = os.path.join(ROOT, "tests", "golden", f"dfnet_grad_{name}_part{i}.npz")
            np.savez_compressed(path, **part)
            print(name, "part", i, len(part) // 4, "tensors", os.path.getsize(path), "bytes")
        print(name, x.shape, "worst fp32_dev %.3g at %s" % worst)


if __name__ == "__main__":
    main()
