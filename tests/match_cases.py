"""Seeded numpy recipes for the coarse matcher's tests (no torch RNG: they reproduce anywhere).

A case = (N, M, C, seed, noise, thr).  Descriptors ~ N(0, 1); three quarters of the 3-D points get a planted partner desc1[perm[i]] = desc0[i] + noise N(0, 1);
weights = uniform(+-1/sqrt(fan_in)) (torch's default Linear init) plus a "dot-product direction" so that the net discriminates the way a trained one does.
tools/gen_match_golden.py runs the reference on these inputs; tests/golden/s2d_*.npz hold its outputs only.
"""
from collections import namedtuple

import numpy as np

MatchCase = namedtuple("MatchCase", "name N M C seed noise thr ties")

CASES = {
    "small": MatchCase("small", 96, 600, 192, 11, 0.25, 0.2, False),
    "c128": MatchCase("c128", 64, 320, 128, 12, 0.25, 0.2, False),
    "c256": MatchCase("c256", 64, 320, 256, 13, 0.25, 0.2, False),
    "ties": MatchCase("ties", 96, 600, 192, 14, 0.25, 0.2, True),
    # no golden file (too large): checked against tests/match_ref.py in fp64
    "mid": MatchCase("mid", 256, 1200, 192, 15, 0.35, 0.2, False),
    "full": MatchCase("full", 1024, 4800, 192, 16, 0.35, 0.2, False),
}
GOLDEN_CASES = ("small", "c128", "c256", "ties")
HIDDEN = 128
PARAM_NAMES = ("mlps.0.weight", "mlps.0.bias", "mlps.2.weight", "mlps.2.bias", "mlps.4.weight", "mlps.4.bias")


def make_weights(C, seed):
    rng = np.random.default_rng(seed + 1000)

    def uni(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return rng.uniform(-b, b, size=shape).astype(np.float32)
    w = {
        "mlps.0.weight": uni((HIDDEN, C), C), "mlps.0.bias": uni((HIDDEN,), C),
        "mlps.2.weight": uni((HIDDEN, HIDDEN), HIDDEN), "mlps.2.bias": uni((HIDDEN,), HIDDEN),
        "mlps.4.weight": uni((1, HIDDEN), HIDDEN), "mlps.4.bias": uni((1,), HIDDEN),
    }
    w["mlps.0.weight"][:16, :] += np.float32(1.0 / C)
    w["mlps.2.weight"][:16, :16] += np.float32(0.15)
    w["mlps.4.weight"][0, :16] += np.float32(0.18)
    w["mlps.4.bias"] -= np.float32(4.0)
    return w


def make_case(case):
    """-> dict(desc0 (N,C), desc1 (M,C), weights {name: array}, thr, planted (N) int64 with -1 = no partner, conf_matrix_gt (N,M) float32)."""
    if isinstance(case, str):
        case = CASES[case]
    rng = np.random.default_rng(case.seed)
    N, M, C = case.N, case.M, case.C
    desc0 = rng.standard_normal((N, C)).astype(np.float32)
    desc1 = rng.standard_normal((M, C)).astype(np.float32)
    n_pl = (3 * N) // 4
    perm = rng.permutation(M)[:n_pl]
    desc1[perm] = desc0[:n_pl] + np.float32(case.noise) * rng.standard_normal((n_pl, C)).astype(np.float32)
    planted = np.full(N, -1, dtype=np.int64)
    planted[:n_pl] = perm
    if case.ties:
        # desc1 rows 10, 11 and 300 become byte-copies of one planted partner (of 3-D row 5): that row ties three columns
        src = planted[5]
        for j in (10, 11, 300):
            hit = np.nonzero(planted == j)[0]
            planted[hit] = -1   # whoever was planted there lost its partner
            desc1[j] = desc1[src]
        # two 3-D rows are byte-copies of each other: their shared partner column ties two rows
        # (the tied rows are scaled so that they keep their columns against the saturated row below, which otherwise wins most columns of the scene)
        desc0[5] *= np.float32(TIE_ROW_SCALE)
        desc0[20] *= np.float32(TIE_ROW_SCALE)
        desc0[21] = desc0[20]
        planted[21] = planted[20]
        # 3-D row 7 is pushed into sigmoid saturation (score exactly 1.0f) for two columns: its partner and a byte-copy of it
        j7 = planted[7]
        free = [j for j in range(M) if j not in set(planted.tolist()) and j not in (10, 11, 300)][0]
        desc1[free] = desc1[j7]
        desc0[7] *= np.float32(SATURATION_SCALE)
    gt = np.zeros((N, M), dtype=np.float32)
    ok = planted >= 0
    gt[np.nonzero(ok)[0], planted[ok]] = 1.0
    return dict(desc0=desc0, desc1=desc1, weights=make_weights(C, case.seed), thr=case.thr, planted=planted, conf_matrix_gt=gt, case=case)


# the factor on desc0[7] of the ties case; tools/gen_match_golden.py asserts that the fp32 reference score is exactly 1.0f for >= 2 columns of that row
SATURATION_SCALE = 5.5
TIE_ROW_SCALE = 2.5
