"""include/nerfloc_cnn.h's arithmetic restated in numpy (fp64): the per-frame encoder DepthFusionNet written from the header's text, with no torch in it.
tests/test_dfnet_cpu.py holds it to the fixtures the reference wrote (1e-12), which proves the header; the GPU tests use it where no fixture exists."""
from __future__ import annotations

import numpy as np

EPS = 1e-5


def _reflect_index(n, pad):
    i = np.arange(-pad, n + pad)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def conv(x, w, stride=1, pad=0, bias=None):
    """x (V, Ci, H, W), w (Co, Ci, k, k): a k x k convolution of stride `stride` over x padded by `pad` with reflect."""
    V, Ci, H, W = x.shape
    Co, _, k, _ = w.shape
    if pad:
        x = x[:, :, _reflect_index(H, pad)][:, :, :, _reflect_index(W, pad)]
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = np.zeros((V, Co, ho, wo))
    for ky in range(k):
        for kx in range(k):
            patch = x[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            y += np.einsum("vchw,oc->vohw", patch, w[:, :, ky, kx])
    return y if bias is None else y + bias[None, :, None, None]


def inorm(x, gamma, beta):
    mean = x.mean(axis=(2, 3), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(2, 3), keepdims=True)   # biased, from the deviations
    return (x - mean) * (gamma[None, :, None, None] / np.sqrt(var + EPS)) + beta[None, :, None, None]


def relu(x):
    return np.maximum(x, 0.0)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def up2(x):
    """bilinear x 2, align_corners: source coordinate = dst (in - 1) / (out - 1)."""
    def axis(n):
        s = np.arange(2 * n) * ((n - 1) / (2 * n - 1))
        i0 = np.minimum(np.floor(s).astype(int), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), s - i0
    y0, y1, ly = axis(x.shape[2])
    x0, x1, lx = axis(x.shape[3])
    ly, lx = ly[None, None, :, None], lx[None, None, None, :]
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def dfnet_forward(cnn_in, weights):
    """cnn_in (V, 12, H, W), weights {state-dict name: array} -> dict(out, x1, x2, x3) in fp64."""
    w = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    x = np.asarray(cnn_in, np.float64)

    def block(x, pre, stride):
        a = relu(inorm(conv(x, w[pre + "conv1.weight"], stride, 1), w[pre + "bn1.weight"], w[pre + "bn1.bias"]))
        b = inorm(conv(a, w[pre + "conv2.weight"], 1, 1), w[pre + "bn2.weight"], w[pre + "bn2.bias"])
        i = x if stride == 1 else inorm(conv(x, w[pre + "downsample.0.weight"], 2, 0), w[pre + "downsample.1.weight"], w[pre + "downsample.1.bias"])
        return relu(b + i)

    def conv_in_elu(x, pre):   # the conv's bias is kept here: InstanceNorm removes it (the library skips it)
        return elu(inorm(conv(x, w[pre + "conv.weight"], 1, 1, w[pre + "conv.bias"]), w[pre + "bn.weight"], w[pre + "bn.bias"]))

    f = "fuse_net."
    c0 = relu(inorm(conv(x, w[f + "conv1.weight"], 2, 2), w[f + "bn1.weight"], w[f + "bn1.bias"]))
    xs = [c0]
    for L in (1, 2, 3):
        xs.append(block(block(xs[-1], f"{f}layer{L}.0.", 2), f"{f}layer{L}.1.", 1))
    _, x1, x2, x3 = xs
    u3 = conv_in_elu(up2(x3), f + "upconv3.conv.")
    i3 = conv_in_elu(np.concatenate([u3, x2], 1), f + "iconv3.")
    u2 = conv_in_elu(up2(i3), f + "upconv2.conv.")
    i2 = conv_in_elu(np.concatenate([u2, x1], 1), f + "iconv2.")
    feats = conv(i2, w[f + "out_conv.weight"], 1, 0, w[f + "out_conv.bias"])
    d = conv(relu(conv(x[:, 3:4], w["depth_skip.0.weight"], 2, 0, w["depth_skip.0.bias"])), w["depth_skip.2.weight"], 2, 0, w["depth_skip.2.bias"])
    out = conv(np.concatenate([d, feats], 1), w["conv_out.weight"], 1, 0, w["conv_out.bias"])
    return {"out": out, "x1": x1, "x2": x2, "x3": x3}
