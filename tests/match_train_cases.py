"""Seeded recipes for the coarse matcher's training tests: the recipes of tests/match_cases.py (descriptors, planted targets, weights) at the smallest shapes
at which the gradient kernels can still go wrong, plus the cotangents of a training step.

A case = a match_cases.MatchCase + g_loss (the cotangent of coarse_loss) + whether score_matrix gets a random cotangent g_score ~ N(0, 1) / (N M) + whether one
3-D row is pushed into sigmoid saturation (score exactly 1.0f in fp32: the focal derivative at p == 1).
tools/gen_match_train_golden.py runs the reference on these inputs; tests/golden/s2d_grad_<case>.npz hold its results only.
Fixture sizes: a file holds fp64 tensors (tests/match_train_ref.py is pinned to them at 1e-9, which fp32 storage cannot carry), and random fp64 does not
compress.  The gradients of mlps.0.weight (128 x C) and mlps.2.weight (128 x 128) alone are 196 KB + 131 KB at C = 192 and 262 KB + 131 KB at C = 256 whatever
N and M are, so no file at these widths fits the 204 KB of the largest score fixture (s2d_small.npz); `one` (C = 32) does.  What N and M add is kept small
instead: M of the `small` recipe is cut to 160 (from 600; five column tiles, 48 row pairs), which leaves 245 KB for desc1's gradient, 147 KB for desc0's and
123 KB of logits — 0.8 MB per `small`-based file, 0.4 to 0.6 MB for the others, every file under the 1-MiB limit.  The `ties` recipe of match_cases needs
M > 300 (it copies desc1 rows 10, 11 and 300), so the saturated case here is `small` with that recipe's saturated row only.  The shape that crosses the row
chunks of the backward pass is `mid`, which has no golden and is checked against tests/match_train_ref.py in fp64 at the flat bar.
"""
from collections import namedtuple

import numpy as np

from . import match_cases as mc

TrainCase = namedtuple("TrainCase", "base g_loss g_score saturate")

_small = mc.CASES["small"]._replace(M=160)
CASES = {
    "small": TrainCase(_small._replace(name="tr_small"), 1.0, False, False),
    "ragged": TrainCase(mc.MatchCase("tr_ragged", 37, 75, 192, 21, 0.25, 0.2, False), 1.0, False, False),
    "c128": TrainCase(mc.MatchCase("tr_c128", 34, 70, 128, 22, 0.25, 0.2, False), 1.0, False, False),
    "c256": TrainCase(mc.MatchCase("tr_c256", 34, 70, 256, 23, 0.25, 0.2, False), 1.0, False, False),
    "ties": TrainCase(_small._replace(name="tr_ties", seed=14), 1.0, False, True),
    "one": TrainCase(mc.MatchCase("tr_one", 1, 1, 32, 24, 0.25, 0.2, False), 1.0, False, False),
    "gscore": TrainCase(_small._replace(name="tr_gscore"), 0.37, True, False),
    # no golden file (too large): checked against tests/match_train_ref.py in fp64
    "mid": TrainCase(mc.CASES["mid"], 1.0, True, False),
}
GOLDEN_CASES = ("small", "ragged", "c128", "c256", "ties", "one", "gscore")
GRAD_NAMES = ("desc0", "desc1") + mc.PARAM_NAMES
SATURATED_ROW = 7


def make_case(name):
    """-> match_cases.make_case(...) plus g_loss (float), g_score ((N, M) float32 or None)."""
    tc = CASES[name]
    c = mc.make_case(tc.base)
    if tc.saturate:
        # the planted pair of row 7 and a byte-copy of its partner saturate (as the `ties` recipe of match_cases, without the rows that need M > 300)
        j7 = int(c["planted"][SATURATED_ROW])
        free = [j for j in range(tc.base.M) if j not in set(c["planted"].tolist())][0]
        c["desc1"][free] = c["desc1"][j7]
        c["desc0"][SATURATED_ROW] *= np.float32(mc.SATURATION_SCALE)
    c["g_loss"] = float(tc.g_loss)
    c["g_score"] = None
    if tc.g_score:
        rng = np.random.default_rng(tc.base.seed + 5000)
        c["g_score"] = (rng.standard_normal((tc.base.N, tc.base.M)) / (tc.base.N * tc.base.M)).astype(np.float32)
    return c
