"""Training-step fixtures of SelfCrossTransformer: the recipes of tests/sct_cases.py unchanged, plus seeded cotangents of the two outputs, and the loader of the
gradient goldens.

g_out0 (B, N0, C), g_out1 (B, N1, C) ~ N(0, 1) from their own stream default_rng(case.seed + 1000), so that the forward recipe's draws stay what they are.
tools/gen_sct_train_golden.py runs the reference's SelfCrossTransformer (eval mode, autograd) on these inputs; tests/golden/sct_grad_*.npz hold its results only, for
the seven C = 64 recipes (the parameter gradients of C >= 128 are 2 - 9 MB: those recipes are checked against tests/sct_train_ref.py instead).
"""
import os

import numpy as np

from tests import sct_cases as sc
from tests.fine_train_cases import split_golden
from tests.sct_cases import CASES, NHEAD, STATE_NAMES  # noqa: F401

GOLDEN_CASES = ("small", "exact", "long", "peaked", "fine64", "swap", "one")
REF_CASES = ("c128", "c192", "c256", "fine")
INPUT_GRADS = ("g_v0", "g_pos0", "g_v1", "g_pos1")
# constructed and never applied: the reference leaves their .grad None
UNUSED = tuple(f"{layer}.norm1.{leaf}" for layer in sc.LAYERS[2:] for leaf in ("weight", "bias"))
PARAM_NAMES = tuple(n for n in STATE_NAMES if n not in UNUSED)


def key(name):
    return name.replace(".", "_")


def cotangents(case):
    rng = np.random.default_rng(case.seed + 1000)
    g0 = rng.standard_normal((case.B, case.N0, case.C)).astype(np.float32)
    g1 = rng.standard_normal((case.B, case.N1, case.C)).astype(np.float32)
    return g0, g1


def make_case(name):
    """sct_cases.make_case plus `g_out0`, `g_out1`."""
    c = sc.make_case(name)
    c["g_out0"], c["g_out1"] = cotangents(c["case"])
    return c


def golden_paths(golden_dir, name, parts):
    return [os.path.join(golden_dir, f"sct_grad_{name}.npz")] + [os.path.join(golden_dir, f"sct_grad_{name}_part{k}.npz") for k in range(1, parts)]


def save_grad_golden(golden_dir, name, tensors):
    files = split_golden(tensors)
    for p, f in zip(golden_paths(golden_dir, name, len(files)), files):
        np.savez_compressed(p, **f)
    return len(files)


def load_grad_golden(golden_dir, name):
    """dict of a case's gradient golden, put together from its files: `L`, INPUT_GRADS, key(parameter name) and `dev_<key>` (the reference's fp32-vs-fp64 deviation)."""
    first = dict(np.load(os.path.join(golden_dir, f"sct_grad_{name}.npz")))
    out = dict(first)
    for p in golden_paths(golden_dir, name, int(first["parts"]))[1:]:
        out.update(np.load(p))
    assert not any("__" in k for k in out), "no tensor of the C = 64 recipes is larger than one file"
    return out
