"""Writes tests/golden/sct_drop_<id>[_part<k>].npz: outputs and GRADIENTS of the reference's SelfCrossTransformer in TRAIN mode, with the library's dropout masks.

Build container only: imports the reference's models/COTR/transformer.py in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE).
For the run, torch.nn.functional.dropout is replaced by a function that multiplies by the numpy masks of tests/sct_dropout_ref.py (the restatement of
csrc/sct_drop.h) for (layer, site) in call order: per layer the attention probabilities (B * 8, Nq, Nk) with index b * 8 + h, then (Nq, B, C) after out_proj,
(Nq, B, F) after the ReLU and (Nq, B, C) after linear2, sequence first.  Asserted: exactly 16 calls with these shapes and the module's p.
The module runs in fp64 and in fp32 with L = sum(g_out0 * out0) + sum(g_out1 * out1) on the recipes and cotangents of tests/sct_train_cases.py.  Each id's files hold
L, out0, out1, the four input gradients and the 48 parameter gradients as the fp32 rounding of the fp64 result, per tensor `dev_<key>` (the reference's own
fp32-versus-fp64 deviation, max |difference| / max |fp64|), p, seed and the kept fraction per site (`kept`, 4 layers x 4 sites).  Asserted per id: every deviation
is at most 3e-5 and tests/sct_dropout_ref.py in fp64 agrees with the reference's fp64 to 1e-9.  The C >= 128 recipes are only measured (their parameter gradients
are 2 - 9 MB).  Nothing of the reference's program text is copied.

    python tools/gen_sct_dropout_golden.py --reference /path/to/NeRF-Loc
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
from gen_sct_train_golden import rel  # noqa: E402
from tests import sct_cases as sc  # noqa: E402
from tests import sct_dropout_ref as dr  # noqa: E402
from tests import sct_train_cases as stc  # noqa: E402


class MaskedDropout:
    """Stands in for torch.nn.functional.dropout during one forward of the reference module."""

    def __init__(self, case, p, seed):
        self.case, self.p, self.seed, self.calls, self.kept = case, p, seed, 0, np.zeros((4, 4))

    def __call__(self, x, p=0.5, training=True, inplace=False):
        c = self.case
        layer, site = divmod(self.calls, 4)
        assert layer < 4 and training and not inplace and abs(p - self.p) < 1e-12, (self.calls, p, training)
        nq, nk = ((c.N0, c.N0), (c.N1, c.N1), (c.N0, c.N1), (c.N1, c.N0))[layer]
        if site == 0:
            assert tuple(x.shape) == (c.B * sc.NHEAD, nq, nk), (self.calls, x.shape)
            m = dr.attn_mask(self.seed, self.p, layer, c.B, nq, nk).reshape(c.B * sc.NHEAD, nq, nk)
        else:
            width = c.F if site == 2 else c.C
            assert tuple(x.shape) == (nq, c.B, width), (self.calls, x.shape)
            m = dr.row_mask(self.seed, self.p, layer, site, c.B, nq, width).transpose(1, 0, 2)   # the reference is sequence first
        self.kept[layer, site] = m.mean()
        self.calls += 1
        return x * (torch.from_numpy(np.ascontiguousarray(m)).to(x.dtype) * dr.scale(self.p))


def run(ref, c, p, seed, dtype):
    case = c["case"]
    m = ref.SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, dropout=p, activation="relu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    m = m.to(dtype).train()
    t = [torch.from_numpy(c[k]).to(dtype).requires_grad_(True) for k in ("v0", "pos0", "v1", "pos1")]
    drop, orig = MaskedDropout(case, p, seed), torch.nn.functional.dropout
    torch.nn.functional.dropout = drop
    try:
        o0, o1 = m(*t)
    finally:
        torch.nn.functional.dropout = orig
    assert drop.calls == 16, drop.calls
    L = (o0 * torch.from_numpy(c["g_out0"]).to(dtype)).sum() + (o1 * torch.from_numpy(c["g_out1"]).to(dtype)).sum()
    L.backward()
    res = {"L": float(L.detach()), "out0": o0.detach().numpy(), "out1": o1.detach().numpy(), "kept": drop.kept}
    res.update({k: x.grad.numpy() for k, x in zip(stc.INPUT_GRADS, t)})
    res.update({n: None if q.grad is None else q.grad.numpy() for n, q in m.named_parameters()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    for gid, (name, p, seed) in {**dr.GOLDENS, **dr.REF_CASES}.items():
        c = stc.make_case(name)
        r64, r32 = run(ref, c, p, seed, torch.float64), run(ref, c, p, seed, torch.float32)
        none = tuple(n for n in sc.STATE_NAMES if r64[n] is None)
        assert none == stc.UNUSED, (gid, none)
        mine = dr.grads(c, p, seed, torch.float64)
        keys = ("out0", "out1") + stc.INPUT_GRADS + stc.PARAM_NAMES
        dev = {k: rel(r32[k], r64[k]) for k in keys}
        rst = max(rel(mine[k], r64[k]) for k in keys)
        kw = max(dev, key=dev.get)
        print(f"{gid} ({name}, p {p}, seed {seed:#x}): L {r64['L']:.6f}; reference fp32 vs fp64 worst {dev[kw]:.2e} ({kw}); restatement fp64 vs reference fp64 "
              f"{rst:.2e}; kept {r64['kept'].min():.4f} .. {r64['kept'].max():.4f}")
        assert dev[kw] <= 3e-5 and rst <= 1e-9 and abs(mine["L"] - r64["L"]) <= 1e-9 * max(1.0, abs(r64["L"])), gid
        if gid not in dr.GOLDENS:
            continue
        tensors = {"L": np.float64(r64["L"]), "p": np.float64(p), "seed": np.uint64(seed), "kept": r64["kept"]}
        for k in keys:
            tensors[stc.key(k)] = r64[k].astype(np.float32)
            tensors["dev_" + stc.key(k)] = np.float64(dev[k])
        n = dr.save_golden(out, gid, tensors)
        for path in dr.golden_paths(out, gid, n):
            assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
        print(f"  wrote {n} file(s)")


if __name__ == "__main__":
    main()
