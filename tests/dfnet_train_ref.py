"""include/nerfloc_cnn_train.h's stage arithmetic restated in numpy (fp64), on top of tests/dfnet_ref.py: the gradients of one reflect-padded convolution, of one
InstanceNorm given the norm the forward kept, and of the bilinear x 2.  No torch in it."""
from __future__ import annotations

import numpy as np

from tests.dfnet_ref import EPS, _reflect_index

PAD = {1: 0, 3: 1, 8: 2}


def conv_backward(x, w, g_y, stride):
    """x (V, Ci, H, W) (a concat already joined), w (Co, Ci, k, k), g_y (V, Co, ho, wo) -> (g_x, g_w) of sum(conv(x, w) * g_y), reflect pad PAD[k]."""
    x, w, g_y = (np.asarray(a, dtype=np.float64) for a in (x, w, g_y))
    V, Ci, H, W = x.shape
    Co, _, k, _ = w.shape
    pad = PAD[k]
    iy, ix = _reflect_index(H, pad), _reflect_index(W, pad)
    xp = x[:, :, iy][:, :, :, ix]
    ho, wo = g_y.shape[2:]
    assert (ho, wo) == ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    g_w, g_xp = np.zeros_like(w), np.zeros_like(xp)
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride))
            g_w[:, :, ky, kx] = np.einsum("vohw,vchw->oc", g_y, xp[sl])
            g_xp[sl] += np.einsum("vohw,oc->vchw", g_y, w[:, :, ky, kx])
    g_x = np.zeros_like(x)   # the fold: every padded position's gradient goes to the pixel it mirrored
    np.add.at(g_x, (slice(None), slice(None), iy[:, None], ix[None, :]), g_xp)
    return g_x, g_w


def make_norm(x, gamma, beta):
    """(V, C, 4) fp32 as the forward keeps it: (mean, gamma / sqrt(var + eps), beta, 1 / sqrt(var + eps)), from fp64 statistics of x (V, C, n)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=2)
    rstd = 1.0 / np.sqrt(((x - mean[..., None]) ** 2).mean(axis=2) + EPS)
    return np.stack([mean, gamma[None] * rstd, np.broadcast_to(beta[None], mean.shape), rstd], axis=2).astype(np.float32)


def act_of(x, nrm, act):
    """act(IN(x)) by the kept norm, fp64: act 0 none, 1 ReLU, 2 ELU."""
    x, nrm = np.asarray(x, dtype=np.float64), np.asarray(nrm, dtype=np.float64)
    y = (x - nrm[..., 0:1]) * nrm[..., 1:2] + nrm[..., 2:3]
    return y if act == 0 else np.maximum(y, 0.0) if act == 1 else np.where(y > 0, y, np.expm1(np.minimum(y, 0.0)))


def instnorm_backward(x, nrm, y, act, g_y):
    """x, g_y (V, C, n), nrm (V, C, 4), y the kept output -> (g_x, g_gamma, g_beta): the header's formulas."""
    x, nrm, g_y = (np.asarray(a, dtype=np.float64) for a in (x, nrm, g_y))
    if act == 0:
        g_z = g_y
    else:
        y = np.asarray(y, dtype=np.float64)
        g_z = g_y * ((y > 0) if act == 1 else np.where(y > 0, 1.0, y + 1.0))
    n = x.shape[2]
    xhat = (x - nrm[..., 0:1]) * nrm[..., 3:4]
    s1, s2 = g_z.sum(axis=2, keepdims=True), (g_z * xhat).sum(axis=2, keepdims=True)
    g_x = nrm[..., 1:2] * (g_z - s1 / n - xhat * (s2 / n))
    return g_x, s2[..., 0].sum(axis=0), s1[..., 0].sum(axis=0)


def up2_backward(g_y):
    """g_y (P, 2 h, 2 w) -> g_x (P, h, w): the transpose of dfnet_ref.up2."""
    g_y = np.asarray(g_y, dtype=np.float64)

    def matrix(n):   # (2 n, n): row o holds the two weights of destination o
        s = np.arange(2 * n) * ((n - 1) / (2 * n - 1))
        i0 = np.minimum(np.floor(s).astype(int), n - 1)
        i1, l = np.minimum(i0 + 1, n - 1), s - i0
        m = np.zeros((2 * n, n))
        np.add.at(m, (np.arange(2 * n), i0), 1 - l)
        np.add.at(m, (np.arange(2 * n), i1), l)
        return m
    return np.einsum("pyx,yh,xw->phw", g_y, matrix(g_y.shape[1] // 2), matrix(g_y.shape[2] // 2))
