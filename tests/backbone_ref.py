"""The arithmetic of include/nerfloc_backbone.h restated in numpy, fp64: what nlb_backbone_forward computes, in the header's words.  Sums are numpy's (the order
of a sum is below fp64's resolution at the bars the tests use).  Inputs are the recipe's fp32 arrays, widened."""
from __future__ import annotations

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
EPS = 1e-5


def conv(x, w, stride, pad):
    """x (V, Cin, h, w), w (O, Cin, k, k): a k x k convolution of stride `stride` over x padded by `pad` with zeros."""
    V, _, h, wd = x.shape
    O, _, k, _ = w.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = np.zeros((V, x.shape[1], h + 2 * pad, wd + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    y = np.zeros((V, O, ho, wo))
    for ky in range(k):
        for kx in range(k):
            patch = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            y += np.einsum("vchw,oc->vohw", patch, w[:, :, ky, kx])
    return y


def fold_bn(w, prefix):
    scale = w[prefix + ".weight"] * (1.0 / np.sqrt(w[prefix + ".running_var"] + EPS))
    return scale, w[prefix + ".bias"] - w[prefix + ".running_mean"] * scale


def bn(x, w, prefix):
    scale, bias = fold_bn(w, prefix)
    return x * scale[None, :, None, None] + bias[None, :, None, None]


def relu(x):
    return np.maximum(x, 0.0)


def maxpool_3_2_1(x):
    V, C, h, wd = x.shape
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    xp = np.full((V, C, h + 2, wd + 2), -np.inf)
    xp[:, :, 1:1 + h, 1:1 + wd] = x
    y = np.full((V, C, ho, wo), -np.inf)
    for ky in range(3):
        for kx in range(3):
            y = np.maximum(y, xp[:, :, ky:ky + 2 * (ho - 1) + 1:2, kx:kx + 2 * (wo - 1) + 1:2])
    return y


def bottleneck(x, w, pre, stride, first):
    a = relu(bn(conv(x, w[pre + ".conv1.weight"], 1, 0), w, pre + ".bn1"))
    b = relu(bn(conv(a, w[pre + ".conv2.weight"], stride, 1), w, pre + ".bn2"))
    i = bn(conv(x, w[pre + ".downsample.0.weight"], stride, 0), w, pre + ".downsample.1") if first else x
    return relu(bn(conv(b, w[pre + ".conv3.weight"], 1, 0), w, pre + ".bn3") + i)


def instance_norm(x):
    mean = x.mean(axis=(2, 3), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(2, 3), keepdims=True)
    return (x - mean) * (1.0 / np.sqrt(var + EPS))


def nearest_index(out, inp):
    """The source index of every destination index: (dst * in) / out in integers."""
    return (np.arange(out) * inp) // out


def up_nearest(x, h, wd):
    return x[:, :, nearest_index(h, x.shape[2])][:, :, :, nearest_index(wd, x.shape[3])]


def backbone_forward(imgs, weights, fp32_constants=True):
    """-> {conv1, layer1, layer2, tap_layer1, tap_layer2} in fp64.  fp32_constants: the image mean and std as the library holds them (rounded to fp32, the
    header's words); False: as an fp64 program holds them, which is what the fixtures' fp64 run did (the two differ by 4e-8 on every tensor)."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in weights.items()}
    x = np.asarray(imgs, dtype=np.float64)
    mean, std = (MEAN.astype(np.float32).astype(np.float64), STD.astype(np.float32).astype(np.float64)) if fp32_constants else (MEAN, STD)
    n = (x - mean[None, :, None, None]) / std[None, :, None, None]
    out = {"conv1": conv(n, w["body.conv1.weight"], 2, 3)}
    x = maxpool_3_2_1(relu(bn(out["conv1"], w, "body.bn1")))
    for b in range(3):
        x = bottleneck(x, w, f"body.layer1.{b}", 1, b == 0)
    x1 = out["tap_layer1"] = x
    for b in range(4):
        x = bottleneck(x, w, f"body.layer2.{b}", 2 if b == 0 else 1, b == 0)
    x2 = out["tap_layer2"] = x
    m2 = instance_norm(conv(x2, w["fpn.inner_blocks.1.0.weight"], 1, 0))
    out["layer2"] = instance_norm(conv(m2, w["fpn.layer_blocks.1.0.weight"], 1, 1))
    m1 = instance_norm(conv(x1, w["fpn.inner_blocks.0.0.weight"], 1, 0)) + up_nearest(m2, x1.shape[2], x1.shape[3])
    out["layer1"] = instance_norm(conv(m1, w["fpn.layer_blocks.0.0.weight"], 1, 1))
    return out
