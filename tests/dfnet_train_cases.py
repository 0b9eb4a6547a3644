"""What the gradient fixtures of the per-frame encoder (tests/golden/dfnet_grad_<recipe>_partN.npz) and their tests share: the recipes (of tests/dfnet_cases.py),
the seeded cotangent, the four biases whose gradient is identically zero, the bar rule, and the loader that joins a recipe's parts.  Shared by
tools/gen_dfnet_train_golden.py, which runs the reference, and by the tests, which run this repository's code.  Nothing here imports torch."""
from __future__ import annotations

import glob
import os

import numpy as np

from tests import dfnet_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = ("wide", "odd5")        # the recipes with a committed fixture
COT_SEED = 7                      # loss = sum(out * cot), cot standard normal
PART_BYTES = 900_000              # raw bytes of gradient (fp32 + int16 remainder) per part file (below the largest fixture already committed)
ZERO_BIASES = tuple(f"fuse_net.{m}.conv.bias" for m in ("upconv3.conv", "iconv3", "upconv2.conv", "iconv2"))   # in front of an InstanceNorm
BAR, GUARD, FACTOR = 1e-4, 1.25e-5, 8.0   # the rule of tests/test_gpu_dfnet.py
# the sweep of the GPU tests: (V, H, W, seed, variant); truth there is the in-repo eager module in fp64 on the CPU
SWEEP = {
    "min32": (1, 32, 32, 11, "plain"),     # 2 x 2 deepest planes: the reflect fold on side 2, up2 from 2 x 2, InstanceNorm over 4 values
    "wide": (2, 32, 48, 12, "plain"),      # two views, not square
    "odd5": (3, 48, 80, 13, "plain"),      # 3 x 5 planes; conv1's plane 23 x 39 = 897: a ragged tile
    "tall": (2, 64, 32, 14, "plain"),
    "scaled": (3, 48, 80, 15, "scaled"),
}


def cotangent(V, H, W, seed=COT_SEED):
    """(V, 32, H/4, W/4) fp64."""
    return np.random.default_rng(seed).standard_normal((V, 32, H // 4, W // 4))


def build(name):
    """-> (cnn_in fp32, weights {name: fp32}, cot fp64) of a SWEEP entry."""
    V, H, W, seed, variant = SWEEP[name]
    return dc.make_input(V, H, W, seed), dc.make_weights(seed, variant), cotangent(V, H, W)


def bar_of(fp32_dev):
    """Per tensor: 1e-4 of max |ref|; 8 x the recorded fp32-against-fp64 deviation of the truth's own program where that exceeds 1.25e-5."""
    return FACTOR * fp32_dev if fp32_dev > GUARD else BAR


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def fixture(name):
    """{grad_<tensor>: fp32 array, fp32_dev_<tensor>: float} of a recipe, its parts joined."""
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", f"dfnet_grad_{name}_part*.npz")))
    assert paths, f"no gradient fixture for {name}"
    out = {}
    for p in paths:
        with np.load(p) as g:
            out.update({k: g[k] for k in g.files})
    return out


def fixture_fp64(g, k):
    """The fp64 gradient the fixture was rounded from, to 2^-40 of its largest value: grad + what the rounding dropped (lo, int16, times lo_scale)."""
    return g["grad_" + k].astype(np.float64) + g["lo_" + k].astype(np.float64) * float(g["lo_scale_" + k])
