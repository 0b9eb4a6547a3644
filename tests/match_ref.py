"""PyTorch-CPU restatement of the coarse matcher's forward (row-chunked, dtype selectable) and of its selection rule.

Test infrastructure, like oracle/: tests/test_match_cpu.py pins it to the goldens the reference itself produced (tests/golden/s2d_*.npz).
"""
import numpy as np
import torch


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def scores(desc0, desc1, weights, dtype=torch.float32, chunk=32, return_logits=False):
    """sigmoid(mlps(desc0[n] * desc1[m])) as an (N, M) numpy array of `dtype`; `chunk` rows of desc0 at a time."""
    d0, d1 = _t(desc0, dtype), _t(desc1, dtype)
    w1, b1 = _t(weights["mlps.0.weight"], dtype), _t(weights["mlps.0.bias"], dtype)
    w2, b2 = _t(weights["mlps.2.weight"], dtype), _t(weights["mlps.2.bias"], dtype)
    w3, b3 = _t(weights["mlps.4.weight"], dtype), _t(weights["mlps.4.bias"], dtype)
    out = []
    with torch.no_grad():
        for a in range(0, d0.shape[0], chunk):
            x = torch.einsum("nc,mc->nmc", d0[a:a + chunk], d1)
            h = torch.relu(torch.nn.functional.linear(x, w1, b1))
            h = torch.relu(torch.nn.functional.linear(h, w2, b2))
            out.append(torch.nn.functional.linear(h, w3, b3).squeeze(-1))
    logit = torch.cat(out, dim=0)
    return (logit if return_logits else torch.sigmoid(logit)).numpy()


def select(score, thr):
    """The reference's rule on a score matrix (sparse_to_dense.py:136-142): match_j (N) int64, -1 = unmatched, else the FIRST column of the row's mask."""
    s = np.asarray(score)
    mask = (s > s.dtype.type(thr)) & (s == s.max(axis=1, keepdims=True)) & (s == s.max(axis=0, keepdims=True))
    any_ = mask.any(axis=1)
    return np.where(any_, mask.argmax(axis=1), -1).astype(np.int64)


def ids_from_match_j(match_j):
    i_ids = np.nonzero(match_j >= 0)[0].astype(np.int64)
    return i_ids, match_j[i_ids].astype(np.int64)


def undecided_rows(score, thr, eps):
    """Rows whose match a score perturbation below eps could change: top-2 gap of the row, distance of the row maximum to thr, or — when the row is within eps
    of winning its arg-max column — the top-2 gap of that column, below eps."""
    s = np.asarray(score, dtype=np.float64)
    N, M = s.shape
    und = np.zeros(N, dtype=bool)
    srt = np.sort(s, axis=1)
    top = srt[:, -1]
    gap = top - srt[:, -2] if M > 1 else np.full(N, np.inf)
    und |= gap < eps
    und |= np.abs(top - thr) < eps
    j = s.argmax(axis=1)
    col = s[:, j]                       # (N, N): column j[i] for every row i
    csrt = np.sort(col, axis=0)
    ctop = csrt[-1]
    cgap = ctop - csrt[-2] if N > 1 else np.full(N, np.inf)
    near_win = (ctop - top) < eps
    und |= near_win & (cgap < eps)
    return und
