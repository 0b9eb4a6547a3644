"""The contracts of include/nerfloc_head.h restated in numpy (the pose solver's is tests/pnp_ref.py on the first `count` matches).

  select_matches   the ordered, fixed-capacity match lists and the device-side info words
  pos_sine_grid    the lin_sine position table of an (H, W) map, in the header's fp32 order of operations
  embed_points     the NeRF embedder; the product x 2^l is exact in fp32, the sine and cosine are taken in fp64 of that fp32 argument and rounded once
"""
import numpy as np


def select_matches(match_j, cap, Mc, kps3d, kps2d, rows_a=None, rows_b=None):
    """-> dict(i_ids, j_ids, b_ids (cap) int64, mkps3d (cap, 3), mkps2d_c (cap, 2), out_a / out_b (cap, C) or None, info (4) int32 = count, total, overflow, 0)."""
    mj = np.asarray(match_j, dtype=np.int64)
    ok = (mj >= 0) & (mj < Mc)                      # an entry outside [0, Mc) is unmatched
    idx = np.nonzero(ok)[0]                         # ascending i: torch.nonzero's order
    total = len(idx)
    count = min(total, cap)
    idx = idx[:count]
    out = {"i_ids": np.zeros(cap, np.int64), "j_ids": np.zeros(cap, np.int64), "b_ids": np.zeros(cap, np.int64),
           "mkps3d": np.zeros((cap, 3), np.float32), "mkps2d_c": np.zeros((cap, 2), np.float32),
           "info": np.array([count, total, int(total > cap), 0], dtype=np.int32)}
    out["i_ids"][:count] = idx
    out["j_ids"][:count] = mj[idx]
    out["mkps3d"][:count] = np.asarray(kps3d, np.float32)[idx]
    if count:
        out["mkps2d_c"][:count] = np.asarray(kps2d, np.float32)[mj[idx]]
    for key, rows in (("out_a", rows_a), ("out_b", rows_b)):
        if rows is None:
            out[key] = None
        else:
            o = np.zeros((cap, rows.shape[1]), np.float32)
            o[:count] = np.asarray(rows, np.float32)[idx]
            out[key] = o
    return out


def pos_sine_grid(H, W, C, dtype=np.float32):
    """(H, W, C): all sines, then all cosines; x before y inside a frequency; every step in `dtype` (fp32: the header's order of operations)."""
    assert C % 4 == 0
    D = C // 4
    f = dtype
    ex = (np.arange(1, W + 1).astype(f) - f(0.5)) / (f(W) + f(1e-6))
    ey = (np.arange(1, H + 1).astype(f) - f(0.5)) / (f(H) + f(1e-6))
    pos = np.stack(np.broadcast_arrays(ex[None, :], ey[:, None]), axis=-1).astype(f)          # (H, W, 2): x, y
    args = [f(i * np.pi) * pos for i in range(1, D + 1)]                                      # float(i pi), one product
    return np.concatenate([np.sin(a) for a in args] + [np.cos(a) for a in args], axis=-1).astype(f)


def embed_points(x, L):
    """x (N, D) fp32 -> (N, 2 D L) fp32."""
    x = np.asarray(x, dtype=np.float32)
    parts = []
    for l in range(L):
        arg = (x * np.float32(2.0 ** l)).astype(np.float32).astype(np.float64)   # exact: a power of two
        parts += [np.sin(arg), np.cos(arg)]
    return np.concatenate(parts, axis=-1).astype(np.float32)
