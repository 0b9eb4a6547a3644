"""fp64 restatement of the fine matcher's two backward stages, written out by hand (no autograd): what nl_fine_match_backward and nl_fine_windows_backward
compute.  Test infrastructure like tests/fine_ref.py; tests/test_fine_train_cpu.py pins it to the gradients the reference itself produced under autograd
(tests/golden/fine_grad_*.npz).
"""
import numpy as np

from tests import fine_ref as fr

W, WW = 7, 49
CLAMP = 1e-10


def _grid():
    g = np.linspace(-1.0, 1.0, W)
    return np.tile(g, W), np.repeat(g, W)   # gx, gy of cell r = wy * 7 + wx


def match_forward(feat_f0, feat_f1, mlp):
    """-> dict(x, a1, a2, logits, heat, coords, var, expec_f), all fp64."""
    f0, f1 = np.asarray(feat_f0, np.float64), np.asarray(feat_f1, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in mlp.items()}
    x = f0[:, None, :] * f1
    a1 = x @ p["mlps.0.weight"].T + p["mlps.0.bias"]
    a2 = np.maximum(a1, 0) @ p["mlps.2.weight"].T + p["mlps.2.bias"]
    logits = (np.maximum(a2, 0) @ p["mlps.4.weight"].T + p["mlps.4.bias"])[..., 0]
    z = logits / np.sqrt(f0.shape[1])
    e = np.exp(z - z.max(axis=1, keepdims=True))
    heat = e / e.sum(axis=1, keepdims=True)
    gx, gy = _grid()
    g = np.stack([gx, gy], axis=1)                      # (49, 2)
    coords = heat @ g
    var = heat @ g ** 2 - coords ** 2
    std = np.sqrt(np.maximum(var, CLAMP)).sum(axis=1)
    return dict(x=x, a1=a1, a2=a2, logits=logits, heat=heat, coords=coords, var=var, expec_f=np.concatenate([coords, std[:, None]], axis=1))


def min_variance(feat_f0, feat_f1, mlp):
    """The smallest per-axis variance of any heat-map (fp64)."""
    return float(match_forward(feat_f0, feat_f1, mlp)["var"].min())


def match_backward(feat_f0, feat_f1, mlp, g_expec):
    """-> dict(expec_f, heat, g_logit, g_x, grads {feat_f0, feat_f1, mlps.*}) in fp64."""
    f0, f1 = np.asarray(feat_f0, np.float64), np.asarray(feat_f1, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in mlp.items()}
    ge = np.asarray(g_expec, np.float64)
    fw = match_forward(f0, f1, mlp)
    heat, coords, var = fw["heat"], fw["coords"], fw["var"]
    gx, gy = _grid()
    g = np.stack([gx, gy], axis=1)
    t = ge[:, 0:1] * gx[None] + ge[:, 1:2] * gy[None]
    # d std / d h[r] = sum over the axes whose variance passes the clamp (>=, torch's clamp gradient) of (g^2 - 2 coord g) / (2 sqrt(var))
    passes = var >= CLAMP
    inv = np.where(passes, 0.5 / np.sqrt(np.where(passes, var, 1.0)), 0.0)          # (M, 2)
    dstd = ((g ** 2)[None] - 2.0 * coords[:, None, :] * g[None]) * inv[:, None, :]   # (M, 49, 2)
    t = t + np.where(ge[:, 2:3] != 0, ge[:, 2:3] * dstd.sum(axis=2), 0.0)
    g_logit = heat * (t - (heat * t).sum(axis=1, keepdims=True)) / np.sqrt(f0.shape[1])
    h1, h2 = np.maximum(fw["a1"], 0), np.maximum(fw["a2"], 0)
    g_a2 = g_logit[..., None] * p["mlps.4.weight"][0] * (fw["a2"] > 0)
    g_a1 = (g_a2 @ p["mlps.2.weight"]) * (fw["a1"] > 0)
    g_x = g_a1 @ p["mlps.0.weight"]
    grads = {
        "feat_f0": (g_x * f1).sum(axis=1), "feat_f1": g_x * f0[:, None, :],
        "mlps.0.weight": np.einsum("mrh,mrc->hc", g_a1, fw["x"]), "mlps.0.bias": g_a1.sum(axis=(0, 1)),
        "mlps.2.weight": np.einsum("mrh,mrk->hk", g_a2, h1), "mlps.2.bias": g_a2.sum(axis=(0, 1)),
        "mlps.4.weight": np.einsum("mr,mrh->h", g_logit, h2)[None], "mlps.4.bias": g_logit.sum(keepdims=True).reshape(1),
    }
    return dict(expec_f=fw["expec_f"], heat=heat, g_logit=g_logit, g_x=g_x, grads=grads)


def windows_backward(feat_f, b_ids, j_ids, stride, proj, g_out):
    """-> {feat_f (B, Cf, Hf, Wf), proj.weight, proj.bias} in fp64 from the cotangent g_out (M, 49, Cout) of the window rows."""
    import torch
    f = np.asarray(feat_f, np.float64)
    B, Cf, Hf, Wf = f.shape
    go = np.asarray(g_out, np.float64)
    wt = np.asarray(proj["proj.weight"], np.float64)
    win = fr.windows(f, b_ids, j_ids, stride, None, torch.float64)          # (M, 49, Cf), zeros outside the map
    rows = go @ wt                                                          # (M, 49, Cf)
    Lx = (Wf - 1) // stride + 1
    j, b = np.asarray(j_ids), np.asarray(b_ids)
    ww = np.arange(WW)
    py = (j // Lx)[:, None] * stride + (ww // W)[None] - W // 2
    px = (j % Lx)[:, None] * stride + (ww % W)[None] - W // 2
    inside = (py >= 0) & (py < Hf) & (px >= 0) & (px < Wf)
    g_map = np.zeros((B, Hf, Wf, Cf))
    bb = np.broadcast_to(b[:, None], py.shape)
    np.add.at(g_map, (bb[inside], py[inside], px[inside]), rows[inside])
    return {"feat_f": g_map.transpose(0, 3, 1, 2), "proj.weight": np.einsum("mro,mrc->oc", go, win), "proj.bias": go.sum(axis=(0, 1))}


def train_step(c):
    """The whole chain feat_f -> windows -> match -> sum(g_expec * expec_f) on a fine_train_cases case: dict(expec_f, heat, g_f1, grads {GRAD_NAMES})."""
    import torch
    case = c["case"]
    f1 = fr.windows(np.asarray(c["feat_f"], np.float64), c["b_ids"], c["j_ids"], case.s, {k: np.asarray(v, np.float64) for k, v in c["proj"].items()}, torch.float64)
    mb = match_backward(c["feat_f0"], f1, c["mlp"], c["g_expec"])
    wb = windows_backward(c["feat_f"], c["b_ids"], c["j_ids"], case.s, c["proj"], mb["grads"]["feat_f1"])
    grads = {k: v for k, v in mb["grads"].items() if k != "feat_f1"}
    grads.update(wb)
    return dict(expec_f=mb["expec_f"], heat=mb["heat"], feat_f1=f1, g_f1=mb["grads"]["feat_f1"], grads=grads)
