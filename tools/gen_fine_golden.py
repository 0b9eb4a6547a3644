"""Writes tests/golden/fine_*.npz: the OUTPUTS of the reference's FinePreprocess and FineMatching on the recipes of tests/fine_cases.py.

Build container only: imports the reference's models/matching/fine_matching.py in place, unmodified — pass its checkout with --reference (default:
$NERFLOC_REFERENCE).  That file imports kornia (two functions) and einops.  The real kornia is used where it is installed; otherwise tools/kornia_standin.py,
written from kornia's documented behaviour, is registered in its place.  The window rows of a case are cut into files below 1 MiB
(tests/fine_cases.py: load_golden).  Which of the two produced a file is recorded in it (`kornia_source`).  Nothing of the
reference's program text is copied; the files hold results, the parameter name lists and shapes.

    python tools/gen_fine_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fine_cases as fc  # noqa: E402
from tests import fine_ref as fr  # noqa: E402


def load_reference(ref_root):
    try:
        import kornia  # noqa: F401
        source = "kornia " + getattr(kornia, "__version__", "?")
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import kornia_standin
        kornia_standin.install()
        source = "stand-in (tools/kornia_standin.py)"
    path = os.path.join(ref_root, "nerf_loc", "models", "matching", "fine_matching.py")
    spec = importlib.util.spec_from_file_location("ref_fine_matching", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, source


def _sd_meta(m):
    sd = m.state_dict()
    return np.array(list(sd.keys())), np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64)


def run(ref, c, loss_type="l2_with_std", training=False):
    case = c["case"]
    pre = ref.FinePreprocess(fc.preprocess_config(case))
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    fm = ref.FineMatching(fc.matching_config(case, loss_type))
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
    pre.train(training)
    fm.train(training)
    data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": torch.from_numpy(c["b_ids"]), "j_ids": torch.from_numpy(c["j_ids"]),
            "mkps2d_c": torch.from_numpy(c["mkps2d_c"]), "expec_f_gt": torch.from_numpy(c["expec_f_gt"])}
    with torch.no_grad():
        f1 = pre(torch.from_numpy(c["feat_f"]), None, data)
        fm(torch.from_numpy(c["feat_f0"]), f1, data)
    return pre, fm, f1, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref, source = load_reference(args.reference)
    print("kornia:", source)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    for name in fc.GOLDEN_CASES:
        c = fc.make_case(name)
        pre, fm, f1, data = run(ref, c)
        f1 = f1.numpy()
        # the reference computes the heat-map but does not keep it: it is recomputed here from the reference's own window rows by tests/fine_ref.py, whose
        # expec_f must then equal the reference's (asserted: the heat-map stored is the one that gives the reference's expectation)
        r32 = fr.match(c["feat_f0"], f1, c["mlp"], c["mkps2d_c"], torch.float32)
        expec = data["expec_f"].numpy()
        assert np.abs(r32["expec_f"] - expec).max() <= 1e-6, name
        d = fr.std_sensitivity(c["feat_f0"], f1, c["mlp"], c["mkps2d_c"])
        share = float((d > 1e-5).mean())
        hmax = r32["heatmap"].max(axis=1)
        r64 = fr.match(c["feat_f0"], f1, c["mlp"], c["mkps2d_c"], torch.float64)
        ref_l1 = float(np.abs(r32["heatmap"].astype(np.float64) - r64["heatmap"]).sum(axis=1).max())
        ref_dc = float(np.abs(r32["expec_f"][:, :2].astype(np.float64) - r64["expec_f"][:, :2]).max())
        print(f"{name}: M {len(c['j_ids'])} rows {f1.shape} heat-map max: median {np.median(hmax):.3f} share > 0.99 {float((hmax > 0.99).mean()):.2f}; "
              f"d_m > 1e-5: {share:.2f} (max {d.max():.2e}); fp32 reference vs fp64: heat-map L1 {ref_l1:.2e} coords {ref_dc:.2e}")
        if name != "peaked":
            assert share <= 0.10, f"{name}: {share:.2f} of the matches have d_m > 1e-5: choose another seed or gain"
        else:
            assert float((hmax > 0.99).mean()) > 0.5, "peaked: most heat-maps must be nearly one-hot"
        # the plain bars (1e-4) must be ten times what fp32 rounding of the reference's own formulation costs, or no fp32 kernel can be held to them
        assert ref_l1 <= 1e-5 and ref_dc <= 1e-5, f"{name}: the recipe's logits are too large for the 1e-4 bars (fp32 reference: {ref_l1:.2e}, {ref_dc:.2e})"
        pn, ps = _sd_meta(pre)
        mn, ms = _sd_meta(fm)
        step = fc.part_rows(f1.shape[2])
        parts = [f1[a:a + step] for a in range(0, f1.shape[0], step)]
        for k, part in enumerate(parts):
            np.savez_compressed(os.path.join(out, f"fine_{name}_rows{k}.npz"), feat_f1=part.astype(np.float32))
        np.savez_compressed(os.path.join(out, f"fine_{name}.npz"), row_parts=np.int64(len(parts)), expec_f=expec.astype(np.float32),
                            mkps2d_f=data["mkps2d_f"].numpy().astype(np.float32), heatmap=r32["heatmap"].astype(np.float32),
                            pre_state_dict_names=pn, pre_state_dict_shapes=ps, match_state_dict_names=mn, match_state_dict_shapes=ms,
                            kornia_source=np.array(source))
    c = fc.make_case(fc.TRAIN_CASE)
    res = {}
    for lt in fc.LOSS_TYPES:
        _, _, _, data = run(ref, c, loss_type=lt, training=True)
        res["fine_loss_" + lt] = np.float64(data["fine_loss"].item())
        print("train", lt, data["fine_loss"].item())
    np.savez_compressed(os.path.join(out, "fine_train.npz"), kornia_source=np.array(source), **res)


if __name__ == "__main__":
    main()
