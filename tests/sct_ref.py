"""The four layers of SelfCrossTransformer restated in plain torch matmuls, in fp32 or fp64, returning every layer's output (written from the description of the
layers, not from the reference's text; tools/gen_sct_golden.py asserts that the fp32 form equals the reference to 2e-6).

layer l of the state dict (tests/sct_cases.py: LAYERS): q = (x + pos_x) Wq^T + bq, k = (mem + pos_mem) Wk^T + bk, v = mem Wv^T + bv; 8 heads of dh = C / 8,
softmax(q k^T / sqrt(dh)) v; out_proj; + x; LayerNorm A; linear2(relu(linear1)); + ; LayerNorm B.  A, B = norm1, norm2 (self layers) or norm2, norm3 (cross layers).
"""
import numpy as np
import torch

from tests import sct_cases as sc


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def layer(state, l, x, pos_x, mem, pos_mem, dtype=torch.float64, nhead=sc.NHEAD):
    """One layer on numpy arrays (B, N, C); returns numpy of `dtype`."""
    name = sc.LAYERS[l]
    cross = l >= 2
    attn = "multihead_attn" if cross else "self_attn"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    g = lambda n: t(state[f"{name}.{n}"])
    x, pos_x, mem, pos_mem = t(x), t(pos_x), t(mem), t(pos_mem)
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
    return _ln(y + f, g(f"{nb}.weight"), g(f"{nb}.bias")).numpy()


def layer_inputs(c, outs, l):
    """(x, pos_x, mem, pos_mem) of layer l given the outputs of the layers before it."""
    if l == 0:
        return c["v0"], c["pos0"], c["v0"], c["pos0"]
    if l == 1:
        return c["v1"], c["pos1"], c["v1"], c["pos1"]
    if l == 2:
        return outs[0], c["pos0"], outs[1], c["pos1"]
    return outs[1], c["pos1"], outs[2], c["pos0"]


def forward(c, dtype=torch.float64):
    """The four layer outputs [v0 after layer 0, v1 after layer 1, v0 after layer 2 (= out0), v1 after layer 3 (= out1)]."""
    outs = []
    for l in range(4):
        outs.append(layer(c["state"], l, *layer_inputs(c, outs, l), dtype=dtype))
    return outs


def max_prob_stats(c):
    """Median and largest row maximum of the softmax of layer 2 (fp64): how peaked a recipe is."""
    outs = forward(c)
    s = c["state"]
    C = c["case"].C
    dh = C // sc.NHEAD
    w, b = s["cross_attn_layer0.multihead_attn.in_proj_weight"].astype(np.float64), s["cross_attn_layer0.multihead_attn.in_proj_bias"].astype(np.float64)
    q = (outs[0] + c["pos0"]) @ w[:C].T + b[:C]
    k = (outs[1] + c["pos1"]) @ w[C:2 * C].T + b[C:2 * C]
    B = q.shape[0]
    q = q.reshape(B, -1, sc.NHEAD, dh).transpose(0, 2, 1, 3) / np.sqrt(dh)
    k = k.reshape(B, -1, sc.NHEAD, dh).transpose(0, 2, 1, 3)
    z = q @ k.transpose(0, 1, 3, 2)
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return float(np.median(p.max(-1))), float(np.abs(z).max())
