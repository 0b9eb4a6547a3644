"""Writes tests/golden/fine_grad_<case>.npz (and _part<k>.npz): the reference's FinePreprocess and FineMatching under autograd on the CPU, on the recipes of
tests/fine_train_cases.py, with modules and inputs in fp64 and again in fp32.

Build container only: imports the reference's models/matching/fine_matching.py in place, unmodified (tools/gen_fine_golden.py: load_reference — kornia, or the
stand-in where it is not installed).  Nothing of the reference's program text is copied.  Chain: feat_f -> FinePreprocess -> FineMatching(feat_f0, .) -> expec_f,
L = sum(g_expec * expec_f).  A case's files hold expec_f and the fp64 gradients of L with respect to feat_f, proj.*, feat_f0 and the six mlps.* (grad_<name>), and
per tensor the reference's own fp32-vs-fp64 deviation max |fp32 - fp64| / max |fp64| (dev_<name>).  `small` also gets the gradients of both training losses in
train mode (loss_<type>, lossgrad_<type>_<name>, lossdev_<type>_<name>).  The fp64 runs have torch's default dtype set to fp64, so that the coordinate grid the
reference builds without a dtype is fp64 too.

A non-zero std cotangent is used only where every heat-map's per-axis variance stays above fine_train_cases.MIN_VARIANCE (asserted): at the 1e-10 clamp the
std's gradient is discontinuous and fp32 disagrees with fp64.

    python tools/gen_fine_train_golden.py --reference /path/to/NeRF-Loc
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fine_cases as fc  # noqa: E402
from tests import fine_train_cases as tc  # noqa: E402
from tests import fine_train_ref as tr  # noqa: E402
from tools.gen_fine_golden import load_reference  # noqa: E402


def run(ref, c, dtype, loss_type=None):
    """loss_type None: eval mode, L = sum(g_expec * expec_f); else train mode, L = fine_loss.  -> (expec_f, L, {name: grad})"""
    case = c["case"]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        pre = ref.FinePreprocess(fc.preprocess_config(case))
        pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
        fm = ref.FineMatching(fc.matching_config(case, loss_type or "l2_with_std"))
        fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
        pre, fm = pre.to(dtype).train(loss_type is not None), fm.to(dtype).train(loss_type is not None)
        feat_f = torch.from_numpy(c["feat_f"]).to(dtype).requires_grad_(True)
        feat_f0 = torch.from_numpy(c["feat_f0"]).to(dtype).requires_grad_(True)
        data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": torch.from_numpy(c["b_ids"]), "j_ids": torch.from_numpy(c["j_ids"]),
                "mkps2d_c": torch.from_numpy(c["mkps2d_c"]).to(dtype), "expec_f_gt": torch.from_numpy(c["expec_f_gt"]).to(dtype)}
        f1 = pre(feat_f, None, data)
        fm(feat_f0, f1, data)
        total = data["fine_loss"] if loss_type else (data["expec_f"] * torch.from_numpy(c["g_expec"]).to(dtype)).sum()
        total.backward()
        grads = {"feat_f": feat_f.grad.numpy(), "feat_f0": feat_f0.grad.numpy()}
        grads.update({n: p.grad.numpy() for n, p in list(pre.named_parameters()) + list(fm.named_parameters())})
        return data["expec_f"].detach().numpy(), float(total.detach()), grads
    finally:
        torch.set_default_dtype(old)


def deviation(a32, a64):
    return float(np.max(np.abs(a32.astype(np.float64) - a64)) / max(float(np.max(np.abs(a64))), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NERFLOC_REFERENCE", ""))
    args = ap.parse_args()
    ref, source = load_reference(args.reference)
    print("kornia:", source)
    torch.set_num_threads(8)
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name in tc.GOLDEN_CASES:
        c = tc.make_case(name)
        r = tr.train_step(c)
        vmin = tr.min_variance(c["feat_f0"], r["feat_f1"], c["mlp"])
        if np.any(c["g_expec"][:, 2] != 0):
            assert vmin > tc.MIN_VARIANCE, f"{name}: per-axis variance down to {vmin:.2e} with a non-zero std cotangent: zero it or change the recipe"
        e64, _, g64 = run(ref, c, torch.float64)
        e32, _, g32 = run(ref, c, torch.float32)
        rec = {"expec_f": e64, "kornia_source": np.array(source), "min_variance": np.float64(vmin)}
        worst = 0.0
        for n in tc.GRAD_NAMES:
            rec["grad_" + tc.key(n)] = g64[n]
            rec["dev_" + tc.key(n)] = np.float64(deviation(g32[n], g64[n]))
            if np.max(np.abs(g64[n])) > 0:
                worst = max(worst, float(rec["dev_" + tc.key(n)]))
        if name == tc.TRAIN_CASE:
            for lt in tc.LOSS_TYPES:
                _, l64, lg64 = run(ref, c, torch.float64, lt)
                _, _, lg32 = run(ref, c, torch.float32, lt)
                rec["loss_" + lt] = np.float64(l64)
                for n in tc.GRAD_NAMES:
                    rec[f"lossgrad_{lt}_{tc.key(n)}"] = lg64[n]
                    rec[f"lossdev_{lt}_{tc.key(n)}"] = np.float64(deviation(lg32[n], lg64[n]))
        files = tc.split_golden(rec)
        sizes = []
        for path, part in zip(tc.golden_paths(out_dir, name, len(files)), files):
            np.savez_compressed(path, **part)
            sizes.append(os.path.getsize(path))
            assert sizes[-1] < (1 << 20), path
        print(f"{name}: M {len(c['j_ids'])} min variance {vmin:.2e} worst deviation {worst:.2e} files {[s // 1024 for s in sizes]} KiB; "
              + " ".join(f"{n}:{float(rec['dev_' + tc.key(n)]):.1e}" for n in tc.GRAD_NAMES))


if __name__ == "__main__":
    main()
