"""The four layers of SelfCrossTransformer under torch autograd in fp64 (or fp32): the restatement of tests/sct_ref.py on tensors that carry gradients, written from
the description there, not from the reference's text (tools/gen_sct_train_golden.py asserts that its fp64 gradients equal the reference's to 1e-9).

L = sum(g_out0 * out0) + sum(g_out1 * out1); `grads` returns dL/d(v0, pos0, v1, pos1) and dL/d(every state tensor) — None for the cross layers' norm1 pair, which
no layer applies.  `layer_grads` does the same for ONE layer on given inputs, so that a deviation can be attributed to its layer.
"""
import numpy as np
import torch

from tests import sct_cases as sc
from tests import sct_train_cases as stc


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def layer_t(state, l, x, pos_x, mem, pos_mem, nhead=sc.NHEAD):
    """Layer l on torch tensors (B, N, C); `state`: {name: tensor}."""
    name = sc.LAYERS[l]
    cross = l >= 2
    attn = "multihead_attn" if cross else "self_attn"
    g = lambda n: state[f"{name}.{n}"]
    B, Nq, C = x.shape
    Nk = mem.shape[1]
    dh = C // nhead
    w, b = g(f"{attn}.in_proj_weight"), g(f"{attn}.in_proj_bias")
    q = (x + pos_x) @ w[:C].T + b[:C]
    k = (mem + pos_mem) @ w[C:2 * C].T + b[C:2 * C]
    v = mem @ w[2 * C:].T + b[2 * C:]
    q = q.view(B, Nq, nhead, dh).transpose(1, 2) * (float(dh) ** -0.5)
    k = k.view(B, Nk, nhead, dh).transpose(1, 2)
    v = v.view(B, Nk, nhead, dh).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    a = (p @ v).transpose(1, 2).reshape(B, Nq, C)
    a = a @ g(f"{attn}.out_proj.weight").T + g(f"{attn}.out_proj.bias")
    na, nb = ("norm2", "norm3") if cross else ("norm1", "norm2")
    y = _ln(x + a, g(f"{na}.weight"), g(f"{na}.bias"))
    f = torch.relu(y @ g("linear1.weight").T + g("linear1.bias")) @ g("linear2.weight").T + g("linear2.bias")
    return _ln(y + f, g(f"{nb}.weight"), g(f"{nb}.bias"))


def _leaf(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)


def _np(t):
    return None if t is None else t.detach().numpy()


def grads(c, dtype=torch.float64):
    """{"L", "out0", "out1", g_v0, g_pos0, g_v1, g_pos1, <state name>: gradient or None} as numpy of `dtype`."""
    state = {n: _leaf(a, dtype) for n, a in c["state"].items()}
    v0, pos0, v1, pos1 = (_leaf(c[k], dtype) for k in ("v0", "pos0", "v1", "pos1"))
    a0 = layer_t(state, 0, v0, pos0, v0, pos0)
    a1 = layer_t(state, 1, v1, pos1, v1, pos1)
    out0 = layer_t(state, 2, a0, pos0, a1, pos1)
    out1 = layer_t(state, 3, a1, pos1, out0, pos0)
    g0, g1 = (torch.from_numpy(c[k]).to(dtype) for k in ("g_out0", "g_out1"))
    L = (g0 * out0).sum() + (g1 * out1).sum()
    L.backward()
    res = {"L": float(L.detach()), "out0": _np(out0), "out1": _np(out1), "g_v0": _np(v0.grad), "g_pos0": _np(pos0.grad), "g_v1": _np(v1.grad), "g_pos1": _np(pos1.grad)}
    res.update({n: _np(t.grad) for n, t in state.items()})
    return res


def layer_grads(c, l, x, pos_x, mem, pos_mem, g_out, dtype=torch.float64):
    """One layer on numpy inputs: {"g_x", "g_pos_x", "g_mem", "g_pos_mem", <the layer's state names>}; for the self layers (l < 2) mem is x and g_x / g_pos_x hold
    the whole gradient (g_mem / g_pos_mem are None)."""
    names = sc.layer_names(sc.LAYERS[l])
    state = {n: _leaf(c["state"][n], dtype) for n in names}
    tx, tpx = _leaf(x, dtype), _leaf(pos_x, dtype)
    tm, tpm = (tx, tpx) if l < 2 else (_leaf(mem, dtype), _leaf(pos_mem, dtype))
    out = layer_t(state, l, tx, tpx, tm, tpm)
    (torch.from_numpy(np.ascontiguousarray(g_out)).to(dtype) * out).sum().backward()
    res = {"g_x": _np(tx.grad), "g_pos_x": _np(tpx.grad), "g_mem": None if l < 2 else _np(tm.grad), "g_pos_mem": None if l < 2 else _np(tpm.grad)}
    res.update({n: _np(t.grad) for n, t in state.items()})
    return res
