"""PyTorch-CPU restatement of the coarse matcher's training step (row-chunked, fp64 by default): logits, the sigmoid focal loss and the gradients of
g_loss * loss + sum(g_score * sigmoid(logits)) with respect to both descriptor sets and the six parameters.

Test infrastructure, like tests/match_ref.py: tests/test_match_train_cpu.py pins it to the goldens the reference itself produced
(tests/golden/s2d_grad_*.npz); the GPU tests use it where a golden would be too large.
"""
import numpy as np
import torch

from .match_cases import PARAM_NAMES

ALPHA, GAMMA = 0.25, 2.0


def focal(logits, target):
    """element-wise sigmoid focal loss, unit anchor weights"""
    p = torch.sigmoid(logits)
    aw = target * ALPHA + (1 - target) * (1 - ALPHA)
    pt = target * (1 - p) + (1 - target) * p
    bce = torch.clamp(logits, min=0) - logits * target + torch.log1p(torch.exp(-torch.abs(logits)))
    return aw * pt.pow(GAMMA) * bce


def train_step(desc0, desc1, weights, target, g_loss=1.0, g_score=None, dtype=torch.float64, chunk=16):
    """-> dict(loss, logits (N, M), grads {name: array}) as numpy arrays of `dtype`; `chunk` rows of desc0 at a time."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    d0, d1 = t(desc0).requires_grad_(True), t(desc1).requires_grad_(True)
    ps = [t(weights[n]).requires_grad_(True) for n in PARAM_NAMES]
    tgt = t(target)
    gs = None if g_score is None else t(g_score)
    N, M = d0.shape[0], d1.shape[0]
    loss = 0.0
    logits = []
    for a in range(0, N, chunk):
        x = torch.einsum("nc,mc->nmc", d0[a:a + chunk], d1)
        h = torch.relu(torch.nn.functional.linear(x, ps[0], ps[1]))
        h = torch.relu(torch.nn.functional.linear(h, ps[2], ps[3]))
        z = torch.nn.functional.linear(h, ps[4], ps[5]).squeeze(-1)
        part = focal(z, tgt[a:a + chunk]).sum() / (N * M)
        total = part * g_loss
        if gs is not None:
            total = total + (torch.sigmoid(z) * gs[a:a + chunk]).sum()
        total.backward()
        loss += float(part.detach())
        logits.append(z.detach())
    grads = {"desc0": d0.grad.numpy(), "desc1": d1.grad.numpy()}
    grads.update({n: p.grad.numpy() for n, p in zip(PARAM_NAMES, ps)})
    return dict(loss=loss, logits=torch.cat(logits, dim=0).numpy(), grads=grads)
