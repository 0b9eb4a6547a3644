"""PyTorch-CPU restatement of the fine matcher's two forwards (dtype selectable) and of its two training losses.

Test infrastructure, like oracle/ and tests/match_ref.py: tests/test_fine_cpu.py pins it to the goldens the reference itself produced (tests/golden/fine_*.npz).
The windows are gathered directly (the reference unfolds the whole map and indexes it: the same values).
"""
import numpy as np
import torch

W = 7
WW = 49


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def windows(feat_f, b_ids, j_ids, stride, proj=None, dtype=torch.float32):
    """(M, 49, Cout) = proj(window) — or the raw (M, 49, Cf) windows with proj=None — of F.unfold(kernel 7, stride, padding 3) + 'n (c ww) l -> n l ww c'."""
    f = _t(feat_f, dtype)
    B, C, Hf, Wf = f.shape
    Lx = (Wf - 1) // stride + 1
    fp = torch.nn.functional.pad(f, (W // 2, W // 2, W // 2, W // 2))
    b, j = torch.from_numpy(np.asarray(b_ids)).long(), torch.from_numpy(np.asarray(j_ids)).long()
    ww = torch.arange(WW)
    py = (j // Lx)[:, None] * stride + (ww // W)[None]      # padded coordinates: + 3 - 3
    px = (j % Lx)[:, None] * stride + (ww % W)[None]
    win = fp[b[:, None], :, py, px]                          # (M, 49, C)
    if proj is None:
        return win.numpy()
    return torch.nn.functional.linear(win, _t(proj["proj.weight"], dtype), _t(proj["proj.bias"], dtype)).numpy()


def padded_cells(Hf, Wf, j_ids, stride):
    """(M, 49) bool: the cells of each window that lie outside the map."""
    Lx = (Wf - 1) // stride + 1
    j = np.asarray(j_ids)
    ww = np.arange(WW)
    py = (j // Lx)[:, None] * stride + (ww // W)[None] - W // 2
    px = (j % Lx)[:, None] * stride + (ww % W)[None] - W // 2
    return (py < 0) | (py >= Hf) | (px < 0) | (px >= Wf)


def match(feat_f0, feat_f1, mlp, mkps2d_c, dtype=torch.float32):
    """-> dict(logits (M,49), heatmap (M,49), expec_f (M,3), mkps2d_f (M,2)) as numpy arrays of `dtype`."""
    f0, f1 = _t(feat_f0, dtype), _t(feat_f1, dtype)
    C = f0.shape[1]
    lin = torch.nn.functional.linear
    with torch.no_grad():
        x = torch.einsum("mc,mrc->mrc", f0, f1)
        h = torch.relu(lin(x, _t(mlp["mlps.0.weight"], dtype), _t(mlp["mlps.0.bias"], dtype)))
        h = torch.relu(lin(h, _t(mlp["mlps.2.weight"], dtype), _t(mlp["mlps.2.bias"], dtype)))
        logits = lin(h, _t(mlp["mlps.4.weight"], dtype), _t(mlp["mlps.4.bias"], dtype)).squeeze(-1)
        heat = torch.softmax((1.0 / C ** 0.5) * logits, dim=1)
        expec = expectation(heat)
        kf = _t(mkps2d_c, dtype) + expec[:, :2] * (W // 2)
    return dict(logits=logits.numpy(), heatmap=heat.numpy(), expec_f=expec.numpy(), mkps2d_f=kf.numpy())


def expectation(heat):
    """(M, 3) = (x, y, std) of (M, 49) heat-maps over linspace(-1, 1, 7)^2, x along the fast axis (a torch tensor in, a torch tensor out)."""
    g = torch.linspace(-1, 1, W, dtype=heat.dtype)
    grid = torch.stack([g[None, :].expand(W, W), g[:, None].expand(W, W)], dim=-1).reshape(1, WW, 2)
    coords = (grid * heat[:, :, None]).sum(dim=1)
    var = (grid ** 2 * heat[:, :, None]).sum(dim=1) - coords ** 2
    std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(-1)
    return torch.cat([coords, std[:, None]], dim=-1)


def std_sensitivity(feat_f0, feat_f1, mlp, mkps2d_c):
    """d_m = |std(fp32) - std(fp64)| per match: what one sample of fp32 rounding noise does to the square root of a difference that can cancel."""
    a = match(feat_f0, feat_f1, mlp, mkps2d_c, torch.float32)["expec_f"][:, 2].astype(np.float64)
    b = match(feat_f0, feat_f1, mlp, mkps2d_c, torch.float64)["expec_f"][:, 2]
    return np.abs(a - b)


def losses(expec_f, expec_f_gt, correct_thr):
    """{'l2': ., 'l2_with_std': .} as the reference computes them in training mode on a batch with at least one correct match."""
    e, g = _t(expec_f, torch.float32), _t(expec_f_gt, torch.float32)
    mask = g.abs().max(dim=1)[0] < correct_thr
    assert bool(mask.any())
    off = ((g[mask] - e[mask, :2]) ** 2).sum(-1)
    inv = 1.0 / torch.clamp(e[:, 2], min=1e-10)
    weight = inv / inv.mean()
    return {"l2": float(off.mean()), "l2_with_std": float((off * weight[mask]).mean())}
