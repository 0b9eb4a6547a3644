"""Drop-in for the reference's coarse matcher, `S2DMatching` (models/matching/sparse_to_dense.py:80-151, used by matcher.py:22,72).

Eval mode on a HIP device is one library call (nl_s2d_match, csrc/s2d.hip): the N x M x C outer product and the two hidden tensors of the reference's
formulation are never materialised.  Training mode, or an input that requires grad, is the library's training step on a HIP device (nl_s2d_forward_train keeps
the logits and writes the focal loss, nl_s2d_backward_train recomputes the hidden activations in row chunks: csrc/s2d_bwd.hip) as one autograd Function;
hip_training = False, or CPU tensors, run the reference's formulation in eager PyTorch in row chunks.  Eval mode on CPU tensors is refused: no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _counted_lib, _lib
from ._packing import (MATCHER_HIDDEN, MATCHER_MLP_PARAMS, PackedCache, check_precision, matcher_mlp_grad_buffers, matcher_mlp_grads_out,
                       pack_matcher_mlp, pack_matcher_mlp_train, require_device)


def sigmoid_focal_loss(logits: torch.Tensor, target: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0) -> torch.Tensor:
    """Element-wise sigmoid focal loss with unit anchor weights (sparse_to_dense.py:14-78); the caller takes the mean."""
    p = torch.sigmoid(logits)
    alpha_w = target * alpha + (1 - target) * (1 - alpha)
    pt = target * (1.0 - p) + (1.0 - target) * p
    bce = torch.clamp(logits, min=0) - logits * target + torch.log1p(torch.exp(-torch.abs(logits)))
    return alpha_w * torch.pow(pt, gamma) * bce


def select_mutual_nearest(score: torch.Tensor, thr: float):
    """The reference's selection (sparse_to_dense.py:136-142): (i_ids, j_ids)."""
    mask = (score > thr) & (score == score.max(dim=1, keepdim=True)[0]) & (score == score.max(dim=0, keepdim=True)[0])
    mask_v, all_j = mask.max(dim=1)
    i_ids = torch.where(mask_v)[0]
    return i_ids, all_j[i_ids]


class _S2DTrainFn(torch.autograd.Function):
    """(desc0, desc1, six parameters) -> (coarse_loss, score_matrix, match_j): the library pair nl_s2d_forward_train / nl_s2d_backward_train.

    target is None in eval mode (no loss: the first output is a zero that carries no gradient).  Parameters that do not require grad get a NULL gradient
    pointer.  The backward pass is not differentiable: a second-order backward raises.
    """

    @staticmethod
    def forward(ctx, mod, target, desc0, desc1, *params):
        lib = _lib.load()
        dev = desc0.device
        d0 = desc0.detach().to(torch.float32).contiguous()
        d1 = desc1.detach().to(torch.float32).contiguous()
        N, M, Cf = d0.shape[0], d1.shape[0], mod.feat_dim
        with torch.cuda.device(dev):
            packed = mod._packed_weights(dev)
            ws = _lib.workspace(lib.nl_s2d_forward_train_workspace_bytes(N, M, Cf), dev, "S2DMatching: unsupported shape")
            scores = torch.empty((N, M), dtype=torch.float32, device=dev)
            logits = torch.empty((N, M), dtype=torch.float32, device=dev)
            loss = torch.zeros((), dtype=torch.float32, device=dev)
            match_j = torch.empty(N, dtype=torch.int32, device=dev)
            match_s = torch.empty(N, dtype=torch.float32, device=dev)
            tgt = None if target is None else target.detach().to(device=dev, dtype=torch.float32).contiguous()
            if tgt is not None and tuple(tgt.shape) != (N, M):
                raise ValueError(f"S2DMatching: conf_matrix_gt must be ({N}, {M})")
            st = _lib.stream(dev)
            _lib.check(lib.nl_s2d_forward_train(packed.data_ptr(), Cf, _lib.PRECISIONS[mod.precision], d0.data_ptr(), N, d1.data_ptr(), M, C.c_float(float(mod.thr)),
                                                _lib.ptr(tgt), scores.data_ptr(), logits.data_ptr(), None if tgt is None else loss.data_ptr(), match_j.data_ptr(),
                                                match_s.data_ptr(), ws.data_ptr(), ws.numel(), st), "nl_s2d_forward_train")
        ctx.mod, ctx.has_target = mod, tgt is not None
        # the images of the weights this forward ran on: a parameter changed in place before backward() must not meet the saved logits
        ctx.packed, ctx.tpacked = packed, mod._packed_train_weights(dev) if any(ctx.needs_input_grad) else None
        ctx.in_dtypes = (desc0.dtype, desc1.dtype)
        ctx.save_for_backward(d0, d1, logits, *([tgt] if tgt is not None else []))
        ctx.mark_non_differentiable(match_j)
        return loss, scores, match_j

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_score, _g_match):
        mod = ctx.mod
        saved = ctx.saved_tensors
        d0, d1, logits = saved[0], saved[1], saved[2]
        tgt = saved[3] if ctx.has_target else None
        lib = _lib.load()
        dev = d0.device
        N, M, Cf = d0.shape[0], d1.shape[0], mod.feat_dim
        with torch.cuda.device(dev):
            packed, tpacked = ctx.packed, ctx.tpacked
            ws = _lib.workspace(lib.nl_s2d_backward_train_workspace_bytes(N, M, Cf), dev, "S2DMatching: shape not supported by the training kernels")
            g_d0 = torch.empty_like(d0)
            g_d1 = torch.empty_like(d1)
            params, g_params = matcher_mlp_grad_buffers(mod, ctx.needs_input_grad[4:], dev)
            gl = None
            if tgt is not None:
                gl = (torch.zeros((), dtype=torch.float32, device=dev) if g_loss is None else g_loss.detach().to(torch.float32)).reshape(1).contiguous()
            gs = None if g_score is None else g_score.detach().to(torch.float32).contiguous()
            st = _lib.stream(dev)
            ptr = _lib.ptr
            _lib.check(lib.nl_s2d_backward_train(packed.data_ptr(), tpacked.data_ptr(), Cf, _lib.PRECISIONS[mod.precision], d0.data_ptr(), N, d1.data_ptr(), M,
                                                 logits.data_ptr(), ptr(tgt), ptr(gl), ptr(gs), g_d0.data_ptr(), g_d1.data_ptr(), *[ptr(g) for g in g_params],
                                                 ws.data_ptr(), ws.numel(), st), "nl_s2d_backward_train")
        return (None, None, g_d0.to(ctx.in_dtypes[0]) if ctx.needs_input_grad[2] else None, g_d1.to(ctx.in_dtypes[1]) if ctx.needs_input_grad[3] else None,
                *matcher_mlp_grads_out(params, g_params))


class S2DMatching(nn.Module, PackedCache):
    """`S2DMatching(feat_dim, thr)` with the reference's parameter names, so `matcher.coarse_matcher.*` of a NeRF-Loc checkpoint loads with strict=True.

    precision: "bf16x3" (default: three-term split-bf16 MFMA, within 1e-4 of the fp32 reference), "fp32" (exact fp32 products) or "bf16" (throughput, not
    held to the parity bar).  want_score_matrix=False leaves data['score_matrix'] = None and skips the N x M output tensor.
    eager_chunk_rows: rows of desc0 per chunk of the eager (training) path.
    hip_training (attribute, default True): on HIP tensors, training mode or a descriptor that requires grad runs the library's training step; False selects the
    eager path (as ConditionalNeRF.hip_training).  CPU tensors always take the eager path there.
    """
    hip_training = True

    def __init__(self, feat_dim, thr=0.1, precision: str = "bf16x3", want_score_matrix: bool = True, eager_chunk_rows: int = 32):
        super().__init__()
        self.mlps = nn.Sequential(nn.Linear(feat_dim, MATCHER_HIDDEN), nn.ReLU(inplace=True), nn.Linear(MATCHER_HIDDEN, MATCHER_HIDDEN), nn.ReLU(inplace=True),
                                  nn.Linear(MATCHER_HIDDEN, 1))
        self.feat_dim = int(feat_dim)
        self.thr = thr
        self.precision = check_precision(precision)
        self.want_score_matrix = bool(want_score_matrix)
        self.eager_chunk_rows = int(eager_chunk_rows)
        self._cache_init()
        self._train_cache = PackedCache()
        self._train_cache._cache_init()

    # ------------------------------------------------------------------ eager path (training / autograd)
    def get_loss(self, conf, conf_gt):
        return sigmoid_focal_loss(conf.unsqueeze(2), conf_gt.unsqueeze(2)).mean()

    def _eager_logits(self, desc0, desc1):
        rows = []
        for a in range(0, desc0.shape[0], self.eager_chunk_rows):
            x = torch.einsum("nc,mc->nmc", desc0[a:a + self.eager_chunk_rows], desc1)
            rows.append(self.mlps(x).squeeze(-1))
        return torch.cat(rows, dim=0)

    # ------------------------------------------------------------------ library path
    def _packed_weights(self, device):
        return pack_matcher_mlp("S2DMatching", self, device)

    def _packed_train_weights(self, device):
        """The training image (the transposed weights of nl_s2d_pack_train_weights), cached like the inference image."""
        return pack_matcher_mlp_train("S2DMatching", self, device)

    def match(self, desc0, desc1, want_scores=None, n=None):
        """The library call: (score_matrix or None, match_j (N) int32 with -1 = unmatched, match_score (N)).  n (default None: every row exists) is a 0-d int32
        DEVICE tensor: only the first n rows of desc0 exist.  nl_s2d_match still scores all N rows (a pair's score has its own bits whatever the other rows are);
        nlk_s2d_select_counted (libnerfloc_counted.so) then replaces the selection: maxima over rows < n, match_j = -1 and match_score = 0 behind n."""
        require_device("S2DMatching", desc0, desc1)
        if desc0.dim() != 2 or desc1.dim() != 2 or desc0.shape[1] != self.feat_dim or desc1.shape[1] != self.feat_dim:
            raise ValueError(f"S2DMatching: descriptors must be (N, {self.feat_dim}) and (M, {self.feat_dim})")
        want = self.want_score_matrix if want_scores is None else bool(want_scores)
        dev = desc0.device
        if n is not None:
            _counted_lib.device_count(n, "S2DMatching.match", dev)
            keep, want = want, True   # the counted selection reads the matrix
        lib = _lib.load()
        d0 = desc0.detach().to(torch.float32).contiguous()
        d1 = desc1.detach().to(torch.float32).contiguous()
        N, M = d0.shape[0], d1.shape[0]
        with torch.cuda.device(dev):
            packed = self._packed_weights(dev)
            ws = _lib.workspace(lib.nl_s2d_min_workspace_bytes(N, M, self.feat_dim, int(want)), dev, "S2DMatching: unsupported shape")
            scores = torch.empty((N, M), dtype=torch.float32, device=dev) if want else None
            match_j = torch.empty(N, dtype=torch.int32, device=dev)
            match_s = torch.empty(N, dtype=torch.float32, device=dev)
            st = _lib.stream(dev)
            _lib.check(lib.nl_s2d_match(packed.data_ptr(), self.feat_dim, _lib.PRECISIONS[self.precision], d0.data_ptr(), N, d1.data_ptr(), M,
                                        C.c_float(float(self.thr)), _lib.ptr(scores), match_j.data_ptr(), match_s.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "nl_s2d_match")
            if n is not None:
                match_j, match_s = _counted_lib.s2d_select_counted(scores, n, self.thr)
                scores = scores if keep else None
        return scores, match_j, match_s

    def forward(self, desc0, desc1, data):
        assert (desc0.shape[0] > 0) and (desc1.shape[0] > 0)
        if self.training or (torch.is_grad_enabled() and (desc0.requires_grad or desc1.requires_grad)):
            if self.hip_training and desc0.is_cuda and desc1.is_cuda:
                if desc0.dim() != 2 or desc1.dim() != 2 or desc0.shape[1] != self.feat_dim or desc1.shape[1] != self.feat_dim:
                    raise ValueError(f"S2DMatching: descriptors must be (N, {self.feat_dim}) and (M, {self.feat_dim})")
                target = data["conf_matrix_gt"] if self.training else None
                # eval mode differentiates the scores with respect to the descriptors only: detached parameters are NULL gradient pointers in the backward call
                params = [self.get_parameter(n) if self.training else self.get_parameter(n).detach() for n in MATCHER_MLP_PARAMS]
                loss, score, match_j = _S2DTrainFn.apply(self, target, desc0, desc1, *params)
                i_ids = torch.nonzero(match_j >= 0).squeeze(1)
                data.update({"i_ids": i_ids, "j_ids": match_j[i_ids].to(torch.int64), "score_matrix": score})
                if self.training:
                    data["coarse_loss"] = loss
                return data
            conf = self._eager_logits(desc0, desc1)
            score = torch.sigmoid(conf)
            i_ids, j_ids = select_mutual_nearest(score, self.thr)
            data.update({"i_ids": i_ids, "j_ids": j_ids, "score_matrix": score})
            if self.training:
                data["coarse_loss"] = self.get_loss(conf, data["conf_matrix_gt"].float())
            return data
        scores, match_j, _ = self.match(desc0, desc1)
        i_ids = torch.nonzero(match_j >= 0).squeeze(1)
        data.update({"i_ids": i_ids, "j_ids": match_j[i_ids].to(torch.int64), "score_matrix": scores})
        return data
