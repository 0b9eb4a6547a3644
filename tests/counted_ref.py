"""Numpy restatement of nlk_s2d_select_counted (include/nerfloc_counted.h), written from the header's text alone: maxima over the rows below the count, the
first column that is over the threshold and both maxima, -1 / 0 behind the count.  tests/test_counted_cpu.py holds it against tests/match_ref.py's rule on the
truncated matrix; the GPU tests hold the library against it."""
import numpy as np


def clamp_count(n, cap):
    return min(int(cap), max(int(n), 0))


def select_counted(scores, n, thr):
    """scores (N, M) fp32 >= 0, n any integer -> match_j (N) int32, match_score (N) fp32."""
    s = np.asarray(scores, dtype=np.float32)
    N, M = s.shape
    n = clamp_count(n, N)
    match_j = np.full(N, -1, dtype=np.int32)
    match_s = np.zeros(N, dtype=np.float32)
    if n == 0:
        return match_j, match_s
    bits = s.view(np.uint32)   # scores >= +0: the order of the values is the order of their bits
    rowmax = bits[:n].max(axis=1)
    colmax = bits[:n].max(axis=0)
    for i in range(n):
        if not rowmax[i:i + 1].view(np.float32)[0] > np.float32(thr):
            continue
        hit = np.nonzero((bits[i] == rowmax[i]) & (bits[i] == colmax))[0]
        if len(hit):
            match_j[i] = hit[0]
            match_s[i] = rowmax[i:i + 1].view(np.float32)[0]
    return match_j, match_s


def tied_scores(N, M, seed):
    """An (N, M) matrix of sigmoid-like scores with planted ties: a few distinct values only, so that rows and columns hold their maxima several times, one row that
    repeats its maximum in two winning columns, and two rows that share a column's maximum."""
    rng = np.random.default_rng(seed)
    s = (rng.integers(1, 8, size=(N, M)) / np.float32(8.0)).astype(np.float32) * np.float32(0.9)
    if N >= 3 and M >= 4:
        s[0, :] = np.float32(0.1); s[0, 1] = s[0, 3] = np.float32(0.95)     # the row maximum twice: the first column wins
        s[1:, 1] = np.minimum(s[1:, 1], np.float32(0.5)); s[1:, 3] = np.minimum(s[1:, 3], np.float32(0.5))
        s[1, 2] = s[2, 2] = np.float32(0.97)                                # two rows share column 2's maximum: both match it
        s[3:, 2] = np.minimum(s[3:, 2], np.float32(0.5))
    return s
