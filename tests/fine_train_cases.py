"""Training-step fixtures of the fine matcher: the recipes of tests/fine_cases.py plus a seeded cotangent of expec_f, and the loader of the gradient goldens.

g_expec (M, 3) ~ N(0, 1).  In `peaked` the std column is zero: 50 of its 96 heat-maps have a per-axis variance down to 3e-16, at the 1e-10 clamp where the std's
gradient is discontinuous and the fp32 reference itself disagrees with fp64 (in a real training step the column is zero too: both losses detach the std weight).
Every other recipe keeps its smallest per-axis variance above MIN_VARIANCE (tools/gen_fine_train_golden.py asserts it, tests/test_fine_train_cpu.py checks it).
tools/gen_fine_train_golden.py runs the reference on these inputs; tests/golden/fine_grad_*.npz hold its results only.
"""
import os

import numpy as np

from tests import fine_cases as fc
from tests.fine_cases import CASES, GOLDEN_CASES, LOSS_TYPES, MLP_NAMES, PROJ_NAMES, TRAIN_CASE, make_case as make_forward_case, scaled  # noqa: F401

GRAD_NAMES = ("feat_f", "feat_f0") + PROJ_NAMES + MLP_NAMES
MIN_VARIANCE = 1e-4          # a non-zero std cotangent is used only where every heat-map's per-axis variance (fp64) stays above this
ZERO_STD_COTANGENT = ("peaked",)
# `flat` (mlps.4.weight = 0): the logits do not depend on the features, so these reference gradients are identically zero and the library's must be too
FLAT_ZERO = ("feat_f", "feat_f0", "proj.weight", "proj.bias", "mlps.0.weight", "mlps.0.bias", "mlps.2.weight", "mlps.2.bias")


def key(name):
    return name.replace(".", "_")


def g_expec(case, M):
    """The cotangent of expec_f for a FineCase with M matches: its own stream, so that the forward recipe's draws stay what they are."""
    rng = np.random.default_rng(1000 + case.seed)
    g = rng.standard_normal((M, 3)).astype(np.float32)
    if case.name in ZERO_STD_COTANGENT:
        g[:, 2] = 0
    return g


def make_case(case):
    """fine_cases.make_case plus `g_expec` (M, 3)."""
    c = make_forward_case(case)
    c["g_expec"] = g_expec(c["case"], len(c["j_ids"]))
    return c


# ---- golden files: no committed file above 1 MiB, so a case's tensors are spread over fine_grad_<case>.npz and fine_grad_<case>_part<k>.npz, and a tensor
# larger than one file is cut, flattened, into <key>__<i> with its shape in <key>__shape
PART_BYTES = 900_000


def split_golden(tensors):
    """{key: array} -> list of {key: array} dicts, each below PART_BYTES of raw data; the first also gets `parts`."""
    pieces = []
    for k, v in tensors.items():
        v = np.asarray(v)
        if v.nbytes <= PART_BYTES or v.ndim == 0:
            pieces.append((k, v))
            continue
        flat, step = v.reshape(-1), PART_BYTES // v.itemsize
        pieces.append((f"{k}__shape", np.array(v.shape, dtype=np.int64)))
        for i, a in enumerate(range(0, flat.size, step)):
            pieces.append((f"{k}__{i}", flat[a:a + step]))
    files, size = [{}], 0
    for k, v in pieces:
        if size + v.nbytes > PART_BYTES and files[-1]:
            files.append({})
            size = 0
        files[-1][k] = v
        size += v.nbytes
    files[0]["parts"] = np.int64(len(files))
    return files


def golden_paths(golden_dir, name, parts):
    return [os.path.join(golden_dir, f"fine_grad_{name}.npz")] + [os.path.join(golden_dir, f"fine_grad_{name}_part{k}.npz") for k in range(1, parts)]


def load_grad_golden(golden_dir, name):
    """dict of a case's gradient golden, put together from its files."""
    first = dict(np.load(os.path.join(golden_dir, f"fine_grad_{name}.npz")))
    raw = dict(first)
    for p in golden_paths(golden_dir, name, int(first["parts"]))[1:]:
        raw.update(np.load(p))
    out, cut = {}, {}
    for k, v in raw.items():
        if "__" in k:
            base, i = k.rsplit("__", 1)
            cut.setdefault(base, {})[i] = v
        else:
            out[k] = v
    for base, d in cut.items():
        out[base] = np.concatenate([d[str(i)] for i in range(len(d) - 1)]).reshape(d["shape"])
    return out
