"""Seeded numpy recipes for the 2-D backbone's fixtures (tests/golden/backbone_*.npz): shared by tools/gen_backbone_golden.py, which runs the reference on them,
and by the tests, which run this repository's code on the same inputs.  Nothing is stored but results: weights and images are regenerated.  No torch here."""
from __future__ import annotations

import numpy as np

RETURN_LAYERS = ["conv1", "layer1", "layer2"]
TENSORS = ("conv1", "layer1", "layer2", "tap_layer1", "tap_layer2")   # the three outputs, then the ResNet's raw layer1 / layer2 in front of the FPN
# name: (V, H, W, fpn_dim, seed, variant) — each the smallest shape at which one thing can go wrong
#   min16   layer2 planes are 2 x 2 under InstanceNorm
#   sq32    the shipped pyramid width
#   odd     planes 17 x 25 / 9 x 13 / 5 x 7: the top-down resize is not x 2, every tile has a tail
#   odd2    odd sizes at a second width
#   wide    the widest pyramid
#   tiles   a layer1 plane of 12 x 44 = 528 pixels: several 128-pixel tiles plus a tail
#   scaled  odd's shape, convolution weights x 4 and BN variances x 16
CASES = {
    "min16": (1, 16, 16, 64, 21, "plain"),
    "sq32": (1, 32, 32, 192, 22, "plain"),
    "odd": (2, 34, 50, 192, 23, "plain"),
    "odd2": (2, 47, 61, 128, 24, "plain"),
    "wide": (1, 64, 96, 256, 25, "plain"),
    "tiles": (1, 48, 176, 192, 26, "plain"),
    "scaled": (2, 34, 50, 192, 27, "scaled"),
}
BN_MEMBERS = ("weight", "bias", "running_mean", "running_var")


def half_up(n):
    return (n - 1) // 2 + 1


def plane_sizes(H, W):
    """((h1, w1), (h2, w2), (h3, w3)): the planes of conv1, layer1 and layer2."""
    h1, w1 = half_up(H), half_up(W)
    h2, w2 = half_up(h1), half_up(w1)
    return (h1, w1), (h2, w2), (half_up(h2), half_up(w2))


def weight_shapes(fpn_dim):
    """[(state-dict name, shape)] of Backbone(['conv1', 'layer1', 'layer2'], use_fpn=True, fpn_dim) in state-dict order: 124 entries."""
    out = []

    def bn(prefix, n):
        out.extend((f"{prefix}.{m}", (n,)) for m in BN_MEMBERS)

    out.append(("body.conv1.weight", (64, 3, 7, 7)))
    bn("body.bn1", 64)
    inplanes = 64
    for layer, planes, blocks in ((1, 64, 3), (2, 128, 4)):
        for b in range(blocks):
            pre = f"body.layer{layer}.{b}"
            out.append((f"{pre}.conv1.weight", (planes, inplanes, 1, 1)))
            bn(f"{pre}.bn1", planes)
            out.append((f"{pre}.conv2.weight", (planes, planes, 3, 3)))
            bn(f"{pre}.bn2", planes)
            out.append((f"{pre}.conv3.weight", (4 * planes, planes, 1, 1)))
            bn(f"{pre}.bn3", 4 * planes)
            if b == 0:
                out.append((f"{pre}.downsample.0.weight", (4 * planes, inplanes, 1, 1)))
                bn(f"{pre}.downsample.1", 4 * planes)
            inplanes = 4 * planes
    out.append(("fpn.inner_blocks.0.0.weight", (fpn_dim, 256, 1, 1)))
    out.append(("fpn.inner_blocks.1.0.weight", (fpn_dim, 512, 1, 1)))
    out.append(("fpn.layer_blocks.0.0.weight", (fpn_dim, fpn_dim, 3, 3)))
    out.append(("fpn.layer_blocks.1.0.weight", (fpn_dim, fpn_dim, 3, 3)))
    return out


def make_weights(seed, fpn_dim, variant="plain"):
    """{state-dict name: fp32 array}: convolutions normal with std sqrt(2 / fan_out); BN weight in [0.75, 1.25], bias 0.1 N, running_mean 0.2 N, running_var in
    [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in weight_shapes(fpn_dim):
        if len(shape) == 4:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
            if variant == "scaled":
                v = v * 4.0
        elif name.endswith(".weight"):
            v = rng.uniform(0.75, 1.25, shape)
        elif name.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape)
        elif name.endswith(".running_mean"):
            v = 0.2 * rng.standard_normal(shape)
        else:
            v = rng.uniform(0.5, 1.5, shape)
            if variant == "scaled":
                v = v * 16.0
        w[name] = v.astype(np.float32)
    return w


def make_images(V, H, W, seed):
    """(V, 3, H, W) fp32, uniform in [0, 1]."""
    return np.random.default_rng(seed + 1000).random((V, 3, H, W)).astype(np.float32)


def build(name):
    """-> (imgs (V, 3, H, W) fp32, weights, fpn_dim)."""
    V, H, W, fpn_dim, seed, variant = CASES[name]
    return make_images(V, H, W, seed), make_weights(seed, fpn_dim, variant), fpn_dim


# ------------------------------------------------------------------------------------------ the fixture files
# A case's arrays lie in tests/golden/backbone_<case>.npz and, where they do not fit below FILE_BUDGET bytes, in backbone_<case>.1.npz, .2.npz, ...; an array
# larger than the budget is cut along its channels into `name@0`, `name@1`, ...  load_golden puts them together again.
FILE_BUDGET = 900_000
NO_TAPS = ("odd2", "wide", "tiles")   # the larger cases carry the three outputs only


def tensors_of(name):
    return TENSORS[:3] if name in NO_TAPS else TENSORS


def split_for_files(arrays):
    """{key: array} -> [{key: array}], each part below FILE_BUDGET bytes (uncompressed), in insertion order."""
    pieces = []
    for k, a in arrays.items():
        a = np.asarray(a)
        n = -(-a.nbytes // FILE_BUDGET)
        if n <= 1:
            pieces.append((k, a))
        else:
            pieces.extend((f"{k}@{i}", part) for i, part in enumerate(np.array_split(a, n, axis=1)))
    files, size = [{}], 0
    for k, a in pieces:
        if size + a.nbytes > FILE_BUDGET and files[-1]:
            files.append({})
            size = 0
        files[-1][k] = a
        size += a.nbytes
    return files


def golden_paths(root, name):
    import os
    paths = [os.path.join(root, "tests", "golden", f"backbone_{name}.npz")]
    while os.path.exists(os.path.join(root, "tests", "golden", f"backbone_{name}.{len(paths)}.npz")):
        paths.append(os.path.join(root, "tests", "golden", f"backbone_{name}.{len(paths)}.npz"))
    return paths


def load_golden(root, name):
    """{key: array} of a case, the cut arrays joined."""
    raw = {}
    for path in golden_paths(root, name):
        with np.load(path) as g:
            raw.update({k: g[k] for k in g.files})
    out, parts = {}, {}
    for k, a in raw.items():
        if "@" in k:
            base, i = k.split("@")
            parts.setdefault(base, {})[int(i)] = a
        else:
            out[k] = a
    for base, d in parts.items():
        out[base] = np.concatenate([d[i] for i in range(len(d))], axis=1)
    return out
