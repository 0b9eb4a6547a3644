"""Writes tests/golden/sct_grad_<case>[_part<k>].npz: the GRADIENTS of the reference's SelfCrossTransformer on the recipes of tests/sct_train_cases.py.

Build container only: imports the reference's models/COTR/transformer.py in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE).
The reference module runs in eval mode (no dropout in effect) under autograd, in fp64 and in fp32, with L = sum(g_out0 * out0) + sum(g_out1 * out1).  Each case's
files hold L, the four input gradients and the 48 parameter gradients as the fp32 rounding of the fp64 result (6e-8, far below the 1e-4 bar), and per tensor
`dev_<key>`: the reference's own fp32-versus-fp64 deviation (max |difference| / max |fp64|).  Asserted per case: exactly the four norm1 tensors of the cross layers
have no gradient, every deviation is at most 3e-5, tests/sct_train_ref.py in fp64 agrees with the reference's fp64 gradients to 1e-9, and `one` has exactly zero
position gradients.  The C = 64 recipes are written; the others (parameter gradients of 2 - 9 MB) are only measured.  Nothing of the reference's program text is copied.

    python tools/gen_sct_train_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_sct_golden import load_reference  # noqa: E402
from tests import sct_cases as sc  # noqa: E402
from tests import sct_train_cases as stc  # noqa: E402
from tests import sct_train_ref as str_  # noqa: E402


def run(ref, c, dtype):
    case = c["case"]
    m = ref.SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, dropout=0.1, activation="relu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    m = m.to(dtype).eval()
    t = [torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in ("v0", "pos0", "v1", "pos1")]
    o0, o1 = m(*t)
    L = (o0 * torch.from_numpy(c["g_out0"]).to(dtype)).sum() + (o1 * torch.from_numpy(c["g_out1"]).to(dtype)).sum()
    L.backward()
    res = {"L": float(L.detach())}
    res.update({k: x.grad.numpy() for k, x in zip(stc.INPUT_GRADS, t)})
    res.update({n: None if p.grad is None else p.grad.numpy() for n, p in m.named_parameters()})
    return res


def rel(a, b):
    s = np.abs(b).max()
    d = np.abs(np.asarray(a, dtype=np.float64) - b).max()
    return float(d / s) if s > 0 else float(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    for name in sc.CASES:
        c = stc.make_case(name)
        r64, r32 = run(ref, c, torch.float64), run(ref, c, torch.float32)
        none = tuple(n for n in sc.STATE_NAMES if r64[n] is None)
        assert none == stc.UNUSED, (name, none)
        mine = str_.grads(c, torch.float64)
        keys = stc.INPUT_GRADS + stc.PARAM_NAMES
        dev = {k: rel(r32[k], r64[k]) for k in keys}
        rst = max(rel(mine[k], r64[k]) for k in keys)
        assert all(mine[n] is None for n in stc.UNUSED)
        kw = max(dev, key=dev.get)
        print(f"{name}: L {r64['L']:.6f}; reference fp32 vs fp64 worst {dev[kw]:.2e} ({kw}); restatement fp64 vs reference fp64 {rst:.2e}")
        assert dev[kw] <= 3e-5 and rst <= 1e-9 and abs(mine["L"] - r64["L"]) <= 1e-9 * max(1.0, abs(r64["L"])), name
        if name == "one":
            assert not r64["g_pos0"].any() and not r64["g_pos1"].any()
        if name not in stc.GOLDEN_CASES:
            continue
        tensors = {"L": np.float64(r64["L"])}
        for k in keys:
            tensors[stc.key(k)] = r64[k].astype(np.float32)
            tensors["dev_" + stc.key(k)] = np.float64(dev[k])
        n = stc.save_grad_golden(out, name, tensors)
        for p in stc.golden_paths(out, name, n):
            assert os.path.getsize(p) < (1 << 20), f"{p} is {os.path.getsize(p)} bytes"
        print(f"  wrote {n} file(s)")


if __name__ == "__main__":
    main()
