"""fp64 numpy restatement of the four contracts of include/nerfloc_app.h (and of the reference's AppearanceEmbedding / AppearanceAdaptLayer, which they restate).

Inputs of any float dtype are taken to fp64 first; nothing here depends on the order of a sum.
"""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def channel_stats(x):
    """x (B, c, ...) in NCHW index order -> (B, 2 c): means, then UNBIASED standard deviations (divisor HW - 1), from the deviations (two passes)."""
    x = _f64(x)
    B, c = x.shape[:2]
    x = x.reshape(B, c, -1)
    mean = x.mean(axis=2)
    dev = x - mean[:, :, None]
    std = np.sqrt((dev * dev).sum(axis=2) / (x.shape[2] - 1))
    return np.concatenate([mean, std], axis=1)


def lrelu(x):
    return np.where(x > 0, x, 0.01 * x)


def adapt_code(emb, target, weights, pre=False):
    """emb (V, E), target (E) or (1, E), weights: the six tensors in state-dict order -> code (V, 2 C); pre=True also returns the two pre-activations."""
    w0, b0, w2, b2, w4, b4 = (_f64(w) for w in weights)
    d = _f64(target).reshape(1, -1) - _f64(emb)
    z1 = d @ w0.T + b0
    z2 = lrelu(z1) @ w2.T + b2
    code = lrelu(z2) @ w4.T + b4
    return (code, z1, z2) if pre else code


def film(x, code, clip=False, raw=False):
    """x (V, ..., C), code (V, 2 C) -> y; raw=True returns the value before the clamp as well."""
    x, code = _f64(x), _f64(code)
    V, C = x.shape[0], x.shape[-1]
    bshape = (V,) + (1,) * (x.ndim - 2) + (C,)
    y0 = code[:, :C].reshape(bshape) * x + code[:, C:].reshape(bshape)
    y = np.clip(y0, 0.0, 1.0) if clip else y0
    return (y, y0) if raw else y


def film_backward(x, code, g_y, clip=False):
    """-> g_x (as x), g_code (V, 2 C): m = (0 <= y <= 1) on the unclamped y with clip, else 1."""
    x, code, g_y = _f64(x), _f64(code), _f64(g_y)
    V, C = x.shape[0], x.shape[-1]
    bshape = (V,) + (1,) * (x.ndim - 2) + (C,)
    g = g_y
    if clip:
        _, y0 = film(x, code, True, raw=True)
        g = np.where((y0 >= 0.0) & (y0 <= 1.0), g_y, 0.0)
    g_x = code[:, :C].reshape(bshape) * g
    g_code = np.concatenate([(g * x).reshape(V, -1, C).sum(axis=1), g.reshape(V, -1, C).sum(axis=1)], axis=1)
    return g_x, g_code


def clip_mask(x, code):
    """True where the rgb layer's y passes unclamped (the fp64 decision)."""
    _, y0 = film(x, code, True, raw=True)
    return (y0 >= 0.0) & (y0 <= 1.0)


def adapt_backward(emb, target, weights, g_code):
    """The MLP's gradients from g_code (V, 2 C): -> dict over embedding, target_embedding (1, E) and the six parameters (state-dict names)."""
    w0, b0, w2, b2, w4, b4 = (_f64(w) for w in weights)
    d = _f64(target).reshape(1, -1) - _f64(emb)
    z1 = d @ w0.T + b0
    h1 = lrelu(z1)
    z2 = h1 @ w2.T + b2
    h2 = lrelu(z2)
    g_code = _f64(g_code)
    g_h2 = g_code @ w4
    g_z2 = g_h2 * np.where(z2 > 0, 1.0, 0.01)
    g_h1 = g_z2 @ w2
    g_z1 = g_h1 * np.where(z1 > 0, 1.0, 0.01)
    g_d = g_z1 @ w0
    return {"embedding": -g_d, "target_embedding": g_d.sum(axis=0, keepdims=True),
            "mlp.0.weight": g_z1.T @ d, "mlp.0.bias": g_z1.sum(axis=0), "mlp.2.weight": g_z2.T @ h1, "mlp.2.bias": g_z2.sum(axis=0),
            "mlp.4.weight": g_code.T @ h2, "mlp.4.bias": g_code.sum(axis=0)}
