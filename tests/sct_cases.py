"""Seeded numpy recipes for the SelfCrossTransformer tests (no torch RNG: they reproduce anywhere).

A case = v0 (B, N0, C), v1 (B, N1, C) ~ N(0, 1), pos0, pos1 ~ U(-1, 1) and the module's 52 tensors in state-dict order: matrices and biases U(+-1/sqrt(fan_in)),
LayerNorm weights 1 + 0.1 N(0, 1) and biases 0.1 N(0, 1) (a dropped affine is seen), and the q and k rows of every in_proj_weight multiplied by sqrt(gain): with
gain 1 every softmax is nearly uniform and a wrong attention kernel would pass; gain 8 gives row maxima of 0.3 - 0.5, gain 30 (`peaked`) nearly one-hot rows with
logits up to +-105.  tools/gen_sct_golden.py runs the reference on these inputs; tests/golden/sct_*.npz hold its outputs only.
"""
import os
from collections import namedtuple

import numpy as np

SctCase = namedtuple("SctCase", "name C F B N0 N1 gain seed")
NHEAD = 8

CASES = {
    "small": SctCase("small", 64, 128, 1, 20, 45, 8.0, 41),
    "c128": SctCase("c128", 128, 256, 2, 33, 65, 8.0, 42),
    "c192": SctCase("c192", 192, 512, 1, 70, 333, 8.0, 43),
    "c256": SctCase("c256", 256, 512, 1, 37, 150, 8.0, 44),
    "exact": SctCase("exact", 64, 128, 3, 64, 128, 8.0, 45),
    "long": SctCase("long", 64, 128, 1, 130, 1100, 8.0, 46),
    "peaked": SctCase("peaked", 64, 128, 1, 40, 200, 30.0, 47),
    "fine": SctCase("fine", 192, 128, 20, 1, 49, 8.0, 48),
    "fine64": SctCase("fine64", 64, 128, 33, 1, 49, 8.0, 49),
    "swap": SctCase("swap", 64, 128, 2, 49, 1, 8.0, 50),
    "one": SctCase("one", 64, 128, 3, 1, 1, 8.0, 51),
}
GOLDEN_CASES = tuple(CASES)
LAYERS = ("self_attn_layer0", "self_attn_layer1", "cross_attn_layer0", "cross_attn_layer1")


def layer_names(layer):
    """The state-dict names of one layer, in state-dict order."""
    cross = layer.startswith("cross")
    attn = "multihead_attn" if cross else "self_attn"
    names = [f"{attn}.in_proj_weight", f"{attn}.in_proj_bias", f"{attn}.out_proj.weight", f"{attn}.out_proj.bias", "linear1.weight", "linear1.bias",
             "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]
    if cross:
        names += ["norm3.weight", "norm3.bias"]
    return [f"{layer}.{n}" for n in names]


STATE_NAMES = tuple(n for layer in LAYERS for n in layer_names(layer))


def _uni(rng, shape, fan_in):
    b = 1.0 / np.sqrt(fan_in)
    return rng.uniform(-b, b, size=shape).astype(np.float32)


def make_case(name):
    """`name`: a key of CASES, or an SctCase (tools/sct_bench.py: the shipped shapes)."""
    c = CASES[name] if isinstance(name, str) else name
    rng = np.random.default_rng(c.seed)
    C, Fh = c.C, c.F
    out = {"case": c}
    out["v0"] = rng.standard_normal((c.B, c.N0, C)).astype(np.float32)
    out["v1"] = rng.standard_normal((c.B, c.N1, C)).astype(np.float32)
    out["pos0"] = rng.uniform(-1, 1, (c.B, c.N0, C)).astype(np.float32)
    out["pos1"] = rng.uniform(-1, 1, (c.B, c.N1, C)).astype(np.float32)
    state = {}
    for n in STATE_NAMES:
        leaf = n.split(".", 1)[1]
        if leaf.endswith("in_proj_weight"):
            w = _uni(rng, (3 * C, C), C)
            w[:2 * C] *= np.float32(np.sqrt(c.gain))
            state[n] = w
        elif leaf.endswith("in_proj_bias"):
            state[n] = _uni(rng, (3 * C,), C)
        elif leaf.endswith("out_proj.weight"):
            state[n] = _uni(rng, (C, C), C)
        elif leaf.endswith("out_proj.bias"):
            state[n] = _uni(rng, (C,), C)
        elif leaf == "linear1.weight":
            state[n] = _uni(rng, (Fh, C), C)
        elif leaf == "linear1.bias":
            state[n] = _uni(rng, (Fh,), C)
        elif leaf == "linear2.weight":
            state[n] = _uni(rng, (C, Fh), Fh)
        elif leaf == "linear2.bias":
            state[n] = _uni(rng, (C,), Fh)
        elif leaf.endswith(".weight"):   # LayerNorm
            state[n] = (1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32)
        else:
            state[n] = (0.1 * rng.standard_normal(C)).astype(np.float32)
    out["state"] = state
    return out


def golden_path(golden_dir, name):
    return os.path.join(golden_dir, f"sct_{name}.npz")


def load_golden(golden_dir, name):
    with np.load(golden_path(golden_dir, name)) as z:
        return {k: z[k] for k in z.files}
