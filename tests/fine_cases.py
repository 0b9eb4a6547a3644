"""Seeded numpy recipes for the fine matcher's tests (no torch RNG: they reproduce anywhere).

A case = a fine feature map (B, Cf, Hf, Wf) ~ N(0, 1), M coarse matches (b_ids, j_ids into the window grid of stride s), the projection Cf -> Cout, the centre
descriptors feat_f0 (M, Cout) ~ N(0, 1), the MLP Cout -> 128 -> 128 -> 1 and the coarse key-points mkps2d_c.  Weights = uniform(+-1/sqrt(fan_in)) (torch's default
Linear init); the MLP's last layer is multiplied by `gain` so that the logits, which the reference divides by sqrt(C) before the softmax, give heat-maps with
structure (gain 1 leaves them uniform to three digits, and a wrong MLP would pass).  tools/gen_fine_golden.py runs the reference on these inputs;
tests/golden/fine_*.npz hold its outputs only.
"""
import os
from collections import namedtuple

import numpy as np

FineCase = namedtuple("FineCase", "name B Cf Cout Hf Wf s M seed ids gain zero_last")

HIDDEN = 128
WINDOW = 7
GAIN = 400.0          # softmax arguments of a few units: heat-map maxima of 0.1 .. 0.9
GAIN_PEAKED = 3500.0  # most heat-maps nearly one-hot (tools/gen_fine_golden.py prints the share)

CASES = {
    "small": FineCase("small", 1, 64, 64, 12, 16, 2, 20, 21, "random", GAIN, False),
    "c192": FineCase("c192", 1, 192, 192, 24, 32, 4, 70, 22, "random", GAIN, False),
    "c256": FineCase("c256", 1, 256, 256, 16, 20, 4, 37, 23, "random", GAIN, False),
    "borders": FineCase("borders", 1, 64, 64, 9, 13, 4, 12, 24, "borders", GAIN, False),
    "odd4": FineCase("odd4", 1, 64, 96, 13, 19, 4, 20, 25, "all", GAIN, False),
    "odd2": FineCase("odd2", 1, 64, 96, 13, 19, 2, 33, 26, "random", GAIN, False),
    "s1": FineCase("s1", 1, 32, 64, 9, 11, 1, 40, 27, "random", GAIN, False),
    "repeat": FineCase("repeat", 2, 64, 64, 12, 16, 2, 24, 28, "repeat", GAIN, False),
    "single": FineCase("single", 1, 64, 64, 12, 16, 2, 1, 29, "random", GAIN, False),
    "peaked": FineCase("peaked", 1, 64, 64, 12, 16, 2, 96, 30, "random", GAIN_PEAKED, False),
    "flat": FineCase("flat", 1, 64, 64, 12, 16, 2, 16, 31, "random", GAIN, True),
}
GOLDEN_CASES = tuple(CASES)
# the `train` golden: the `small` inputs with these ground-truth offsets, both losses
TRAIN_CASE, TRAIN_CORRECT_THR = "small", 1.0
LOSS_TYPES = ("l2", "l2_with_std")
PROJ_NAMES = ("proj.weight", "proj.bias")
MLP_NAMES = ("mlps.0.weight", "mlps.0.bias", "mlps.2.weight", "mlps.2.bias", "mlps.4.weight", "mlps.4.bias")


def grid_shape(Hf, Wf, s):
    """(Ly, Lx) of F.unfold(kernel 7, stride s, padding 3)."""
    return (Hf - 1) // s + 1, (Wf - 1) // s + 1


def preprocess_config(case):
    return {"fine_concat_coarse_feat": False, "fine_window_size": WINDOW, "in_channels_coarse": 2 * case.Cf, "in_channels_fine": case.Cf,
            "out_channels": case.Cout}


def matching_config(case, loss_type="l2_with_std"):
    return {"correct_thr": TRAIN_CORRECT_THR, "loss_type": loss_type, "feat_dim": case.Cout}


def _uni(rng, shape, fan_in):
    b = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-b, b, size=shape).astype(np.float32)


def _ids(case, rng):
    Ly, Lx = grid_shape(case.Hf, case.Wf, case.s)
    L = Ly * Lx
    if case.ids == "borders":   # the four corners, the middle of the four edges, their inner neighbours: padded cells on every side, corners with 33 of 49 padded
        ys, xs = (0, Ly // 2, Ly - 1), (0, Lx // 2, Lx - 1)
        j = [y * Lx + x for y in ys for x in xs] + [Lx + 1, L - Lx - 2, 1]
        j = np.array(j[:case.M], dtype=np.int64)
    elif case.ids == "all":     # every window of the grid once (exercises the Lx formula at every position), in a shuffled order
        assert case.M == L, (case.M, L)
        j = rng.permutation(L).astype(np.int64)
    elif case.ids == "repeat":  # a few windows many times
        j = rng.integers(0, L, size=5)[rng.integers(0, 5, size=case.M)].astype(np.int64)
    else:
        j = rng.integers(0, L, size=case.M).astype(np.int64)
    b = rng.integers(0, case.B, size=len(j)).astype(np.int64)
    return b, j


def make_case(case):
    """-> dict(feat_f (B,Cf,Hf,Wf), b_ids, j_ids (M) int64, stride_coarse, stride_fine, proj {name: array}, feat_f0 (M,Cout), mlp {name: array}, mkps2d_c (M,2),
    expec_f_gt (M,2), case)."""
    if isinstance(case, str):
        case = CASES[case]
    rng = np.random.default_rng(case.seed)
    feat_f = rng.standard_normal((case.B, case.Cf, case.Hf, case.Wf)).astype(np.float32)
    b_ids, j_ids = _ids(case, rng)
    M, C = len(j_ids), case.Cout
    proj = {"proj.weight": _uni(rng, (C, case.Cf), case.Cf), "proj.bias": _uni(rng, (C,), case.Cf)}
    feat_f0 = rng.standard_normal((M, C)).astype(np.float32)
    mlp = {
        "mlps.0.weight": _uni(rng, (HIDDEN, C), C), "mlps.0.bias": _uni(rng, (HIDDEN,), C),
        "mlps.2.weight": _uni(rng, (HIDDEN, HIDDEN), HIDDEN), "mlps.2.bias": _uni(rng, (HIDDEN,), HIDDEN),
        "mlps.4.weight": _uni(rng, (1, HIDDEN), HIDDEN) * np.float32(case.gain), "mlps.4.bias": _uni(rng, (1,), HIDDEN),
    }
    if case.zero_last:
        mlp["mlps.4.weight"][:] = 0
    _, Lx = grid_shape(case.Hf, case.Wf, case.s)
    stride_fine = 2
    mkps2d_c = np.stack([(j_ids % Lx), (j_ids // Lx)], axis=1).astype(np.float32) * np.float32(case.s * stride_fine)
    expec_f_gt = rng.uniform(-1.5, 1.5, size=(M, 2)).astype(np.float32)   # about a third of the rows fall outside correct_thr = 1
    return dict(feat_f=feat_f, b_ids=b_ids, j_ids=j_ids, stride_coarse=case.s * stride_fine, stride_fine=stride_fine, proj=proj, feat_f0=feat_f0, mlp=mlp,
                mkps2d_c=mkps2d_c, expec_f_gt=expec_f_gt, case=case)


def scaled(name, M, Hf, Wf, B=1):
    """The recipe `name` at another size (tools/fine_bench.py: the shipped shape)."""
    return CASES[name]._replace(M=M, Hf=Hf, Wf=Wf, B=B, ids="random")


# ---- golden files: no committed file above 1 MiB, so the reference's window rows (M, 49, Cout) of a case are cut into parts of whole matches
PART_BYTES = 900_000


def part_rows(Cout):
    return max(1, PART_BYTES // (WINDOW * WINDOW * Cout * 4))


def load_golden(golden_dir, name):
    """dict of tests/golden/fine_<name>.npz with `feat_f1` put together from fine_<name>_rows<k>.npz."""
    g = dict(np.load(os.path.join(golden_dir, f"fine_{name}.npz")))
    parts = [np.load(os.path.join(golden_dir, f"fine_{name}_rows{k}.npz"))["feat_f1"] for k in range(int(g["row_parts"]))]
    g["feat_f1"] = np.concatenate(parts, axis=0)
    return g
