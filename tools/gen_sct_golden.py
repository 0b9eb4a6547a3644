"""Writes tests/golden/sct_*.npz: the OUTPUTS of the reference's SelfCrossTransformer on the recipes of tests/sct_cases.py.

Build container only: imports the reference's models/COTR/transformer.py in place, unmodified — pass its checkout with --reference (default: $NERFLOC_REFERENCE).
Each file holds the two outputs in fp32, the state dict's name and shape lists and the reference's own fp32-versus-fp64 deviation.  Two conditions are asserted per
case: that deviation is at most 1e-5 of each output's largest magnitude (so a 1e-4 bar can be held by an fp32 kernel), and tests/sct_ref.py in fp32 is within 2e-6
of the reference (so its fp64 form may stand in for the reference where a test needs a single layer).  Nothing of the reference's program text is copied.

    python tools/gen_sct_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sct_cases as sc  # noqa: E402
from tests import sct_ref as sr  # noqa: E402


def load_reference(ref_root):
    path = os.path.join(ref_root, "nerf_loc", "models", "COTR", "transformer.py")
    spec = importlib.util.spec_from_file_location("ref_cotr_transformer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, c, dtype):
    case = c["case"]
    m = ref.SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, dropout=0.1, activation="relu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    m = m.to(dtype).eval()
    with torch.no_grad():
        o0, o1 = m(*[torch.from_numpy(c[k]).to(dtype) for k in ("v0", "pos0", "v1", "pos1")])
    return m, o0.numpy(), o1.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    bad = []
    for name in sc.GOLDEN_CASES:
        c = sc.make_case(name)
        m, o0, o1 = run(ref, c, torch.float32)
        _, d0, d1 = run(ref, c, torch.float64)
        sd = m.state_dict()
        assert list(sd.keys()) == list(sc.STATE_NAMES), name
        r32 = sr.forward(c, torch.float32)
        dev = [float(np.abs(o.astype(np.float64) - d).max() / np.abs(d).max()) for o, d in ((o0, d0), (o1, d1))]
        rst = [float(np.abs(r.astype(np.float64) - o).max() / np.abs(o).max()) for r, o in ((r32[2], o0), (r32[3], o1))]
        pmed, zmax = sr.max_prob_stats(c)
        print(f"{name}: scale {np.abs(d0).max():.2f} / {np.abs(d1).max():.2f}; reference fp32 vs fp64 {dev[0]:.2e} / {dev[1]:.2e}; restatement fp32 vs reference "
              f"{rst[0]:.2e} / {rst[1]:.2e}; layer 2 softmax: median row maximum {pmed:.3f}, largest |logit| {zmax:.1f}")
        if max(dev) > 1e-5 or max(rst) > 2e-6:
            bad.append(name)
        names = np.array(list(sd.keys()))
        shapes = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64)
        path = sc.golden_path(out, name)
        np.savez_compressed(path, out0=o0.astype(np.float32), out1=o1.astype(np.float32), state_dict_names=names, state_dict_shapes=shapes,
                            ref_fp32_vs_fp64=np.array(dev, dtype=np.float64))
        assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
    assert not bad, f"cases outside the recipe's conditions: {bad}"


if __name__ == "__main__":
    main()
