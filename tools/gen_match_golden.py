"""Writes tests/golden/s2d_*.npz: the OUTPUTS of the reference's S2DMatching on the recipes of tests/match_cases.py.

Build container only: imports the reference's models/matching/sparse_to_dense.py in place, unmodified (it needs torch only) — pass its checkout with
--reference (default: $NERFLOC_REFERENCE).  Nothing of the reference's program text is copied; the files hold results, the parameter name list and shapes.

    python tools/gen_match_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import match_cases as mc  # noqa: E402


def load_reference(ref_root):
    path = os.path.join(ref_root, "nerf_loc", "models", "matching", "sparse_to_dense.py")
    spec = importlib.util.spec_from_file_location("ref_sparse_to_dense", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, name, training=False):
    c = mc.make_case(name)
    case = c["case"]
    m = ref.S2DMatching(case.C, thr=case.thr)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    m.train(training)
    data = {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"])}
    with torch.no_grad():
        m(torch.from_numpy(c["desc0"]), torch.from_numpy(c["desc1"]), data)
    return c, m, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    for name in mc.GOLDEN_CASES:
        c, m, data = run(ref, name)
        s = data["score_matrix"].numpy()
        sd = m.state_dict()
        if name == "ties":
            assert int((s[7] == np.float32(1.0)).sum()) >= 2, "ties case: row 7 must saturate for at least two columns"
        np.savez_compressed(os.path.join(out, f"s2d_{name}.npz"), score_matrix=s.astype(np.float32), i_ids=data["i_ids"].numpy(),
                            j_ids=data["j_ids"].numpy(), state_dict_names=np.array(list(sd.keys())),
                            state_dict_shapes=np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64))
        print(name, s.shape, "matches", len(data["i_ids"]), "score range", float(s.min()), float(s.max()))
    c, m, data = run(ref, "small", training=True)
    np.savez_compressed(os.path.join(out, "s2d_train.npz"), coarse_loss=np.float64(data["coarse_loss"].item()))
    print("train coarse_loss", data["coarse_loss"].item())


if __name__ == "__main__":
    main()
