"""Writes tests/golden/s2d_grad_<case>.npz: the reference's S2DMatching in train mode on the CPU under autograd, on the recipes of tests/match_train_cases.py,
in fp32 and again with module and inputs in fp64.

Build container only: imports the reference's models/matching/sparse_to_dense.py in place, unmodified — pass its checkout with --reference
(default: $NERFLOC_REFERENCE).  Nothing of the reference's program text is copied; a file holds the fp64 loss, logits and gradients of
g_loss * coarse_loss + sum(g_score * score_matrix) with respect to desc0, desc1 and the six parameters, and per tensor the reference's own fp32-vs-fp64
deviation max |fp32 - fp64| / max |fp64| (dev_<name>), which must stay below 1e-5: a recipe that exceeds it is to be changed, not the bar.

    python tools/gen_match_train_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import match_train_cases as tc  # noqa: E402
from tools.gen_match_golden import load_reference  # noqa: E402

MAX_REFERENCE_DEVIATION = 1e-5


def run(ref, c, dtype):
    case = c["case"]
    m = ref.S2DMatching(case.C, thr=case.thr)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    m = m.to(dtype).train()
    d0 = torch.from_numpy(c["desc0"]).to(dtype).requires_grad_(True)
    d1 = torch.from_numpy(c["desc1"]).to(dtype).requires_grad_(True)
    data = {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"]).to(dtype)}
    logits = {}
    hook = m.mlps.register_forward_hook(lambda mod, inp, out: logits.update(z=out.detach().squeeze(-1).clone()))
    m(d0, d1, data)
    hook.remove()
    total = data["coarse_loss"] * c["g_loss"]
    if c["g_score"] is not None:
        total = total + (data["score_matrix"] * torch.from_numpy(c["g_score"]).to(dtype)).sum()
    total.backward()
    out = {"loss": data["coarse_loss"].detach().numpy(), "logits": logits["z"].numpy(), "score": data["score_matrix"].detach().numpy(),
           "desc0": d0.grad.numpy(), "desc1": d1.grad.numpy()}
    out.update({n: p.grad.numpy() for n, p in m.named_parameters()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name in tc.GOLDEN_CASES:
        c = tc.make_case(name)
        r32, r64 = run(ref, c, torch.float32), run(ref, c, torch.float64)
        if tc.CASES[name].saturate:
            assert int((r32["score"][tc.SATURATED_ROW] == np.float32(1.0)).sum()) >= 2, "saturated case: row 7 must reach score 1.0f for two columns"
        rec = {"loss": np.float64(r64["loss"]), "logits": r64["logits"]}
        worst = 0.0
        for k in ("loss", "logits") + tc.GRAD_NAMES:
            dev = float(np.max(np.abs(r32[k].astype(np.float64) - r64[k])) / max(np.max(np.abs(r64[k])), 1e-300))
            rec["dev_" + k.replace(".", "_")] = np.float64(dev)
            worst = max(worst, dev)
            assert dev <= MAX_REFERENCE_DEVIATION, f"{name}: reference fp32-vs-fp64 deviation of {k} is {dev:.3e} > {MAX_REFERENCE_DEVIATION}: change the recipe"
        for k in tc.GRAD_NAMES:
            rec["grad_" + k.replace(".", "_")] = r64[k]
        path = os.path.join(out_dir, f"s2d_grad_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, r64["logits"].shape, "loss", float(r64["loss"]), "worst deviation", f"{worst:.2e}", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
