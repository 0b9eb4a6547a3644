"""The dropout masks of the SelfCrossTransformer training step restated in numpy, bit for bit (csrc/sct_drop.h is the one device definition), and the four layers
under torch autograd with those masks applied (tests/sct_train_ref.py's formulation plus the four sites).

Generator: Philox4x32-10 with the published constants, key = (seed & 0xffffffff, seed >> 32).  One call = four 32-bit words = eight 16-bit fields = 4 x 2 elements:
    counter = (major >> 2, minor >> 1, group, 4 * layer + site);  element (major, minor) = bits [16 * (minor & 1), + 16) of word major & 3
    site 0 (attention probabilities): major = key, minor = query, group = 8 * batch item + head
    site 1 (out_proj's output), 2 (ReLU'd hidden rows), 3 (linear2's output): major = row flattened over the batch (b * Nq + q), minor = column, group = 0
kept <=> field >= threshold(p) = round-half-even(65536 p) (at most 65535); kept values are multiplied by scale(p) = 65536 / (65536 - threshold): the keep probability
is exactly 1 - threshold / 65536, and the scale its inverse.
"""
import os

import numpy as np
import torch

from tests import sct_cases as sc
from tests.fine_train_cases import split_golden
from tests.sct_train_ref import _leaf, _ln, _np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (broadcast) and a two-word key -> the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _U32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    return min(int(np.rint(np.float64(np.float32(p)) * 65536.0)), 65535)


def keep_probability(p):
    return 1.0 - threshold(p) / 65536.0


def scale(p):
    return float(np.float32(65536.0 / (65536 - threshold(p))))


def site_mask(seed, p, layer, site, group, major, minor):
    """bool array (broadcast of group, major, minor): True = kept."""
    group, major, minor = (np.asarray(a, dtype=np.int64) for a in np.broadcast_arrays(group, major, minor))
    w = philox4x32_10(major >> 2, minor >> 1, group, np.int64(4 * layer + site), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    word = np.choose(major & 3, w)
    field = (word >> (16 * (minor & 1)).astype(np.uint32)) & np.uint32(0xFFFF)
    return field >= np.uint32(threshold(p))


def attn_mask(seed, p, layer, B, Nq, Nk, b=None, q=None, k=None):
    """(B, 8, Nq, Nk) keep mask of site 0, or its cut at the index arrays b / q / k."""
    b = np.arange(B) if b is None else np.asarray(b)
    q = np.arange(Nq) if q is None else np.asarray(q)
    k = np.arange(Nk) if k is None else np.asarray(k)
    g = (8 * b[:, None] + np.arange(8)[None, :])[:, :, None, None]
    return site_mask(seed, p, layer, 0, g, k[None, None, None, :], q[None, None, :, None])


def row_mask(seed, p, layer, site, B, Nq, width, rows=None):
    """(B, Nq, width) keep mask of site 1..3 (row = b * Nq + q), or (len(rows), width) for the flattened rows asked for."""
    r = np.arange(B * Nq) if rows is None else np.asarray(rows)
    m = site_mask(seed, p, layer, site, 0, r[:, None], np.arange(width)[None, :])
    return m.reshape(B, Nq, width) if rows is None else m


def layer_masks(seed, p, layer, B, Nq, Nk, C, F):
    return (attn_mask(seed, p, layer, B, Nq, Nk), row_mask(seed, p, layer, 1, B, Nq, C), row_mask(seed, p, layer, 2, B, Nq, F), row_mask(seed, p, layer, 3, B, Nq, C))


def layer_t(state, l, x, pos_x, mem, pos_mem, p, seed, nhead=sc.NHEAD):
    """tests/sct_train_ref.layer_t with the four sites of layer l dropped: x, mem (B, N, C) torch tensors."""
    name = sc.LAYERS[l]
    cross = l >= 2
    attn = "multihead_attn" if cross else "self_attn"
    g = lambda n: state[f"{name}.{n}"]
    B, Nq, C = x.shape
    Nk = mem.shape[1]
    dh = C // nhead
    Fh = g("linear1.weight").shape[0]
    s = scale(p)
    m0, m1, m2, m3 = (torch.from_numpy(m).to(x.dtype) * s for m in layer_masks(seed, p, l, B, Nq, Nk, C, Fh))
    w, b = g(f"{attn}.in_proj_weight"), g(f"{attn}.in_proj_bias")
    q = (x + pos_x) @ w[:C].T + b[:C]
    k = (mem + pos_mem) @ w[C:2 * C].T + b[C:2 * C]
    v = mem @ w[2 * C:].T + b[2 * C:]
    q = q.view(B, Nq, nhead, dh).transpose(1, 2) * (float(dh) ** -0.5)
    k = k.view(B, Nk, nhead, dh).transpose(1, 2)
    v = v.view(B, Nk, nhead, dh).transpose(1, 2)
    pr = torch.softmax(q @ k.transpose(-1, -2), dim=-1) * m0
    a = (pr @ v).transpose(1, 2).reshape(B, Nq, C)
    a = (a @ g(f"{attn}.out_proj.weight").T + g(f"{attn}.out_proj.bias")) * m1
    na, nb = ("norm2", "norm3") if cross else ("norm1", "norm2")
    y = _ln(x + a, g(f"{na}.weight"), g(f"{na}.bias"))
    h = torch.relu(y @ g("linear1.weight").T + g("linear1.bias")) * m2
    f = (h @ g("linear2.weight").T + g("linear2.bias")) * m3
    return _ln(y + f, g(f"{nb}.weight"), g(f"{nb}.bias"))


def grads(c, p, seed, dtype=torch.float64):
    """tests/sct_train_ref.grads with dropout (p, seed): {"L", "out0", "out1", g_v0, g_pos0, g_v1, g_pos1, <state name>: gradient or None}."""
    state = {n: _leaf(a, dtype) for n, a in c["state"].items()}
    v0, pos0, v1, pos1 = (_leaf(c[k], dtype) for k in ("v0", "pos0", "v1", "pos1"))
    a0 = layer_t(state, 0, v0, pos0, v0, pos0, p, seed)
    a1 = layer_t(state, 1, v1, pos1, v1, pos1, p, seed)
    out0 = layer_t(state, 2, a0, pos0, a1, pos1, p, seed)
    out1 = layer_t(state, 3, a1, pos1, out0, pos0, p, seed)
    g0, g1 = (torch.from_numpy(c[k]).to(dtype) for k in ("g_out0", "g_out1"))
    L = (g0 * out0).sum() + (g1 * out1).sum()
    L.backward()
    res = {"L": float(L.detach()), "out0": _np(out0), "out1": _np(out1), "g_v0": _np(v0.grad), "g_pos0": _np(pos0.grad), "g_v1": _np(v1.grad), "g_pos1": _np(pos1.grad),
           "mid0": _np(a0), "mid1": _np(a1)}
    res.update({n: _np(t.grad) for n, t in state.items()})
    return res


def layer_grads(c, l, x, pos_x, mem, pos_mem, g_out, p, seed, dtype=torch.float64):
    """tests/sct_train_ref.layer_grads with dropout (p, seed)."""
    names = sc.layer_names(sc.LAYERS[l])
    state = {n: _leaf(c["state"][n], dtype) for n in names}
    tx, tpx = _leaf(x, dtype), _leaf(pos_x, dtype)
    tm, tpm = (tx, tpx) if l < 2 else (_leaf(mem, dtype), _leaf(pos_mem, dtype))
    out = layer_t(state, l, tx, tpx, tm, tpm, p, seed)
    (torch.from_numpy(np.ascontiguousarray(g_out)).to(dtype) * out).sum().backward()
    res = {"g_x": _np(tx.grad), "g_pos_x": _np(tpx.grad), "g_mem": None if l < 2 else _np(tm.grad), "g_pos_mem": None if l < 2 else _np(tpm.grad)}
    res.update({n: _np(t.grad) for n, t in state.items()})
    return res


# ------------------------------------------------------------------------------------------ fixtures (tools/gen_sct_dropout_golden.py)
# golden id -> (recipe of tests/sct_cases.py, p, seed); a seed is replaced (and the replacement recorded here) only if it puts the reference's own fp32 deviation
# beyond 3e-5
GOLDENS = {
    "small": ("small", 0.1, 0x5C7D0001),
    "small_p50": ("small", 0.5, 0x5C7D0002),
    "long": ("long", 0.1, 0x5C7D0003),
    "peaked": ("peaked", 0.1, 0x5C7D0004),
    "fine64": ("fine64", 0.1, 0x5C7D0005),
    "swap": ("swap", 0.1, (0x9E3779B9 << 32) | 0x5C7D0006),   # a seed with a high word
}
REF_CASES = {"c128": ("c128", 0.1, 0x5C7D0011), "c192": ("c192", 0.1, 0x5C7D0012), "fine": ("fine", 0.1, 0x5C7D0013)}


def golden_paths(golden_dir, gid, parts):
    return [os.path.join(golden_dir, f"sct_drop_{gid}.npz")] + [os.path.join(golden_dir, f"sct_drop_{gid}_part{k}.npz") for k in range(1, parts)]


def save_golden(golden_dir, gid, tensors):
    files = split_golden(tensors)
    for path, f in zip(golden_paths(golden_dir, gid, len(files)), files):
        np.savez_compressed(path, **f)
    return len(files)


def load_golden(golden_dir, gid):
    """dict of one golden, put together from its files: L, out0, out1, the input gradients, key(parameter name), dev_<key>, p, seed, kept."""
    first = dict(np.load(os.path.join(golden_dir, f"sct_drop_{gid}.npz")))
    out = dict(first)
    for path in golden_paths(golden_dir, gid, int(first["parts"]))[1:]:
        out.update(np.load(path))
    assert not any("__" in k for k in out), "no tensor of the C = 64 recipes is larger than one file"
    return out
