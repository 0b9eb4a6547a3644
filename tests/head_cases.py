"""Seeded numpy recipes for the tests of the whole localisation head (nerf_loc_amd/matcher.py) and of the head library's entry points (no torch RNG: they
reproduce anywhere).

A head case = everything `Matcher.forward(data)` reads, built from the recipes the stages already have:
  - tests/match_cases.py: descriptors ~ N(0, 1) with three quarters of the 3-D points given a planted partner among the coarse cells, and `make_weights` for BOTH
    matcher MLPs (coarse and fine);
  - tests/sct_cases.py: the two transformers' 52 tensors each, default-initialised from numpy seeds (dim_feedforward 512 and 128, q / k gain 1);
  - the fine map ~ N(0, 1) in NHWC, the projection Cf -> C uniform(+-1/sqrt(fan_in)), one 2-D key point per coarse cell at its place on the fine map, position
    rows ~ U(-1, 1);
  - for training mode: the planted pairs as `pairs_gt`, ground-truth projections within +-1.5 fine pixels of the partner's cell, `conf_matrix_gt`.
The transformers mix every descriptor with its whole set, so a planted pair comes out of them less alike than it went in: `noise` is smaller than in the coarse
matcher's own recipes.  tools/gen_head_golden.py runs the reference's Matcher on these inputs and refuses a recipe with an
undecided row, an fp32 / fp64 disagreement or fewer than 8 matches; tests/golden/head_*.npz hold its outputs only.
"""
import os
from collections import namedtuple

import numpy as np

from tests import match_cases as mc
from tests import sct_cases as sc

HeadCase = namedtuple("HeadCase", "name C N Hc Wc Hf Wf seed noise")
STRIDE_COARSE, STRIDE_FINE = 8, 4
WINDOW = 7
THR = 0.2   # Matcher builds S2DMatching(hidden_dim, thr=0.2)
LOSS_TYPE = "l2_with_std"

CASES = {
    "head64": HeadCase("head64", 64, 60, 6, 8, 12, 16, 71, 0.05),
    "head192": HeadCase("head192", 192, 96, 10, 12, 20, 24, 72, 0.05),
}
GOLDEN_CASES = tuple(CASES)
PREFIXES = ("coarse_transformer", "coarse_matcher", "fine_preprocess", "fine_transformer", "fine_matcher")

# shapes of the position-table and embedder goldens (tests/golden/head_pos.npz)
POS_SHAPES = ((1, 1), (3, 5), (7, 7), (30, 40))
POS_CHANNELS = (64, 192)
EMBED_L = 32
EMBED_SPECIAL = (0.0, 1.0, -1.0, 1e-3, -1e-3, 1.5, -1.5)


class Args:
    """What Matcher's constructor reads of the reference's config."""
    fine_matching_loss_type = LOSS_TYPE


def embed_points_input(n):
    """(n, 3) fp32 in [-1.5, 1.5]; the first values are EMBED_SPECIAL (0, +-1, +-1e-3, +-1.5)."""
    rng = np.random.default_rng(90 + n)
    x = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    flat = x.reshape(-1)
    k = min(len(EMBED_SPECIAL), flat.size)
    flat[:k] = np.array(EMBED_SPECIAL[:k], dtype=np.float32)
    return flat.reshape(n, 3)


def _uni(rng, shape, fan_in):
    b = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-b, b, size=shape).astype(np.float32)


def make_case(name):
    """-> dict(case, data {key: numpy array or int}, state {118 names: arrays}, planted (N) int64)."""
    c = CASES[name] if isinstance(name, str) else name
    C, N, Mc = c.C, c.N, c.Hc * c.Wc
    m = mc.make_case(mc.MatchCase(c.name, N, Mc, C, c.seed, c.noise, THR, False))
    rng = np.random.default_rng(c.seed + 500)
    stride = c.Hf // c.Hc   # fine cells per coarse cell: 2 in the test cases (stride_coarse 8), 4 at the shipped shape of tools/head_bench.py (16)
    assert (c.Hf - 1) // stride + 1 == c.Hc and (c.Wf - 1) // stride + 1 == c.Wc
    cell = np.arange(Mc)
    kps2d = np.stack([(cell % c.Wc) * stride, (cell // c.Wc) * stride], axis=1).astype(np.float32)
    planted = m["planted"]
    ok = np.nonzero(planted >= 0)[0]
    proj_gt = rng.uniform(-40.0, 40.0, size=(N, 2)).astype(np.float32)
    proj_gt[ok] = kps2d[planted[ok]] + rng.uniform(-1.5, 1.5, size=(len(ok), 2)).astype(np.float32)
    data = {
        "desc_3d": m["desc0"], "desc_2d_coarse": m["desc1"],
        "pos_emd_3d": rng.uniform(-1, 1, (N, C)).astype(np.float32), "pos_emd_2d": rng.uniform(-1, 1, (Mc, C)).astype(np.float32),
        "desc_3d_fine": rng.standard_normal((N, C)).astype(np.float32),
        "kps3d": rng.uniform(-1, 1, (N, 3)).astype(np.float32), "kps2d": kps2d,
        "feat_fine": rng.standard_normal((1, c.Hf, c.Wf, C)).astype(np.float32),
        "feat_coarse": rng.standard_normal((1, c.Hc, c.Wc, C)).astype(np.float32),
        "stride_coarse": STRIDE_FINE * stride, "stride_fine": STRIDE_FINE,
        # training mode
        "conf_matrix_gt": m["conf_matrix_gt"], "pairs_gt": np.stack([ok, planted[ok]]).astype(np.int64), "kps3d_proj_gt": proj_gt,
    }
    state = {}
    for prefix, F, seed in (("coarse_transformer", 512, c.seed + 1), ("fine_transformer", 128, c.seed + 2)):
        st = sc.make_case(sc.SctCase(c.name, C, F, 1, 1, 1, 1.0, seed))["state"]
        state.update({f"{prefix}.{k}": v for k, v in st.items()})
    state.update({f"coarse_matcher.{k}": v for k, v in m["weights"].items()})
    state.update({f"fine_matcher.{k}": v for k, v in mc.make_weights(C, c.seed + 3).items()})
    state["fine_preprocess.proj.weight"] = _uni(rng, (C, C), C)
    state["fine_preprocess.proj.bias"] = _uni(rng, (C,), C)
    return {"case": c, "data": data, "state": state, "planted": planted}


INPUT_GRADS = ("desc_3d", "desc_2d_coarse", "desc_3d_fine", "feat_fine")   # the four inputs whose gradients the training goldens hold


def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(golden_dir(), f"head_{name}.npz")) as z:
        return {k: z[k] for k in z.files}
