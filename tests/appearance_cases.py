"""Recipes of the appearance-adaptation tests (tests/test_appearance_cpu.py, tests/test_gpu_appearance.py) and of tools/gen_appearance_golden.py.

Inputs are regenerated from the seeds below, never stored; tests/golden/app_*.npz hold what the reference's AppearanceEmbedding / AppearanceAdaptLayer make of them
in fp64.  The generator refuses a recipe whose clip or LeakyReLU decisions are not safe by 1e-5 (see its docstring), so the seeds here are ones it accepted.
"""
import os
from collections import namedtuple

import numpy as np

EMB_DIM = 128   # appearance_emb_dim of every shipped configuration (2 x 64 conv1 channels); the adapt cases use it whatever their C
HIDDEN = 64

StatsCase = namedtuple("StatsCase", "name B c H W channels_last kind seed")
STATS_CASES = {c.name: c for c in (
    StatsCase("plain", 3, 64, 12, 20, False, "normal", 11),
    StatsCase("offset", 2, 8, 24, 40, False, "offset", 12),      # mean 100, sigma 0.01: E[x^2] - E[x]^2 in fp32 is off by more than the value
    StatsCase("relu", 2, 16, 7, 9, False, "relu", 13),           # half the values exactly 0, an odd plane (no 16-byte loads)
    StatsCase("two", 2, 64, 1, 2, False, "normal", 14),          # HW = 2: the smallest plane with a standard deviation
    StatsCase("one_image", 1, 64, 64, 80, False, "relu", 15),    # B = 1, two segments per plane
    StatsCase("odd_c", 2, 5, 6, 10, True, "normal", 16),         # channels_last with C % 4 != 0
)}

AdaptCase = namedtuple("AdaptCase", "name V H W C is_rgb emb_scale seed")
ADAPT_CASES = {c.name: c for c in (
    AdaptCase("c192", 3, 5, 7, 192, False, 1.0, 21),
    AdaptCase("c64", 3, 5, 7, 64, False, 1.0, 22),
    AdaptCase("rgb", 3, 5, 7, 3, True, 1.0, 23),
    AdaptCase("rgb2", 3, 9, 13, 3, True, 1.0, 24),
    AdaptCase("one_view", 1, 5, 7, 64, False, 1.0, 25),
    AdaptCase("scaled", 3, 5, 7, 64, False, 10.0, 26),           # embeddings x 10: a and b are large
)}
PARAM_NAMES = ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias")
GRAD_NAMES = ("x", "embedding", "target_embedding") + PARAM_NAMES   # the nine gradients of sum(g_y * y)
SAFE_MARGIN = 1e-5   # what the generator demands of clip and LeakyReLU decisions


class Args:
    """What the two constructors read of the reference's config."""
    def __init__(self, dim=EMB_DIM):
        self.appearance_emb_dim = dim


def stats_values(kind, shape, rng):
    if kind == "offset":
        return (100.0 + 0.01 * rng.standard_normal(shape)).astype(np.float32)
    x = rng.standard_normal(shape).astype(np.float32)
    return np.maximum(x, np.float32(0)) if kind == "relu" else x


def make_stats_case(name):
    """-> dict(case, conv1 (B, c, H, W) fp32 in NCHW index order; channels_last cases are laid out by the caller)."""
    c = STATS_CASES[name]
    rng = np.random.default_rng(c.seed)
    return {"case": c, "conv1": stats_values(c.kind, (c.B, c.c, c.H, c.W), rng)}


def stats_plane(HW, c, B, seed, kind="relu"):
    """(B, c, HW) fp32 for the plane-size sweeps, held to the restatement."""
    return stats_values(kind, (B, c, HW), np.random.default_rng(seed))


def make_state(C, rng, E=EMB_DIM):
    """The six tensors of AppearanceAdaptLayer.mlp in state-dict order: nn.Linear's scale, and the last bias lifted by 1 on its `a` half (a near 1, b near 0)."""
    def lin(o, i):
        k = 1.0 / np.sqrt(i)
        return rng.uniform(-k, k, size=(o, i)).astype(np.float32), rng.uniform(-k, k, size=(o,)).astype(np.float32)
    w0, b0 = lin(HIDDEN, E)
    w2, b2 = lin(HIDDEN, HIDDEN)
    w4, b4 = lin(2 * C, HIDDEN)
    b4[:C] += np.float32(1.0)
    return dict(zip(PARAM_NAMES, (w0, b0, w2, b2, w4, b4)))


def make_adapt_case(name):
    """-> dict(case, x (V, H, W, C), embedding (V, E), target_embedding (1, E), state {name: array}, g_y (V, H, W, C)), all fp32."""
    c = ADAPT_CASES[name]
    rng = np.random.default_rng(c.seed)
    shape = (c.V, c.H, c.W, c.C)
    x = rng.uniform(0.0, 1.0, size=shape).astype(np.float32) if c.is_rgb else rng.standard_normal(shape).astype(np.float32)
    emb = (c.emb_scale * rng.standard_normal((c.V, EMB_DIM))).astype(np.float32)
    target = (c.emb_scale * rng.standard_normal((1, EMB_DIM))).astype(np.float32)
    state = make_state(c.C, rng)
    g_y = rng.standard_normal(shape).astype(np.float32)
    return {"case": c, "x": x, "embedding": emb, "target_embedding": target, "state": state, "g_y": g_y}


def film_inputs(V, HW, C, seed, rgb=False):
    """x, code, g_y for the shape sweeps held to the restatement: code's `a` half near 1.  For rgb the values that land within SAFE_MARGIN of a clip boundary in fp64
    are moved off it (x is nudged), so the clipped set is the same in fp32 and fp64."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.0, 1.0, size=(V, HW, C)) if rgb else rng.standard_normal((V, HW, C))).astype(np.float32)
    code = (0.4 * rng.standard_normal((V, 2 * C))).astype(np.float32)
    code[:, :C] += np.float32(1.0)
    g_y = rng.standard_normal((V, HW, C)).astype(np.float32)
    if rgb:
        for _ in range(8):
            y = code[:, None, :C].astype(np.float64) * x + code[:, None, C:].astype(np.float64)
            near = (np.abs(y) < 10 * SAFE_MARGIN) | (np.abs(y - 1.0) < 10 * SAFE_MARGIN)
            if not near.any():
                break
            x = np.where(near, x + np.float32(1e-3), x).astype(np.float32)
        else:
            raise AssertionError("film_inputs: could not move the values off the clip boundaries")
    return x, code, g_y


def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(golden_dir(), f"app_{name}.npz")) as z:
        return {k: z[k] for k in z.files}
