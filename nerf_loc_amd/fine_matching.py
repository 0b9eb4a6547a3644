"""Drop-ins for the reference's fine matcher, `FinePreprocess` and `FineMatching` (models/matching/fine_matching.py:10-76 and :79-207, used by matcher.py:101-124).

Eval mode on a HIP device is one library call each (nl_fine_windows / nl_fine_match, csrc/fine.hip): the unfolded fine map, the M x 49 x C products and the hidden
activations of the reference's formulation are never materialised.  Training mode, or an input that requires grad, is the library's training step on a HIP device
(csrc/fine_bwd.hip): each forward is one autograd Function around the same forward call (FineMatching keeps the heat-map) and nl_fine_windows_backward /
nl_fine_match_backward, which recompute the hidden activations, keep nothing per pair and are bit-reproducible; both losses stay PyTorch on the (M, 3) expec_f.
hip_training = False, CPU tensors or `fine_concat_coarse_feat=True` run the reference's formulation in eager PyTorch, with the M windows gathered directly instead
of unfolding the whole map.  Eval mode on CPU tensors is refused: no CPU fallback.  kornia is not needed.
"""
from __future__ import annotations

import math
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._packing import (MATCHER_HIDDEN, MATCHER_MLP_PARAMS, PackedCache, check_precision, matcher_mlp_grad_buffers, matcher_mlp_grads_out, new_train_cache,
                       pack_matcher_mlp, pack_matcher_mlp_train, require_device)


def gather_windows(feat_f1, b_ids, j_ids, stride, window=7):
    """(M, window^2, C): rows [b_ids, j_ids] of `rearrange(F.unfold(feat_f1, window, stride=stride, padding=window // 2), 'n (c ww) l -> n l ww c')` without
    forming the unfolded map; differentiable with respect to feat_f1."""
    B, C, Hf, Wf = feat_f1.shape
    Lx = (Wf - 1) // stride + 1
    half = window // 2
    fp = F.pad(feat_f1, (half, half, half, half))
    ww = torch.arange(window * window, device=feat_f1.device)
    j = j_ids.long()
    py = (j // Lx)[:, None] * stride + (ww // window)[None]   # padded coordinates
    px = (j % Lx)[:, None] * stride + (ww % window)[None]
    return fp[b_ids.long()[:, None], :, py, px]


class FinePreprocess(nn.Module, PackedCache):
    """`FinePreprocess(config)` with the reference's config keys and parameter names (`proj.*`, or `down_proj.*` / `merge_feat.*` with
    fine_concat_coarse_feat), so `matcher.fine_preprocess.*` of a NeRF-Loc checkpoint loads with strict=True.

    precision: "bf16x3" (default, within 1e-4 of the fp32 reference), "fp32" (exact fp32 products) or "bf16" (throughput, no bar).
    hip_training (attribute): on HIP tensors, training mode or a map that requires grad runs the library's training step; False selects the eager path
    (as S2DMatching.hip_training).  CPU tensors and fine_concat_coarse_feat=True always take the eager path there.
    """
    hip_training = True

    def __init__(self, config, precision: str = "bf16x3"):
        super().__init__()
        self._train_cache = new_train_cache()
        self.config = config
        self.cat_c_feat = config["fine_concat_coarse_feat"]
        self.W = config["fine_window_size"]
        in_channels_coarse, in_channels_fine = config["in_channels_coarse"], config["in_channels_fine"]
        self.in_channels_fine = int(in_channels_fine)
        self.out_channels = int(config["out_channels"])
        if self.cat_c_feat:
            self.down_proj = nn.Linear(in_channels_coarse, in_channels_fine, bias=True)
            self.merge_feat = nn.Linear(2 * in_channels_fine, self.out_channels, bias=True)
        else:
            self.proj = nn.Linear(in_channels_fine, self.out_channels, bias=True)
        self.precision = check_precision(precision)
        self._cache_init()
        self._reset_parameters()

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")

    # ------------------------------------------------------------------ eager path (training / autograd / concatenated coarse features)
    def _eager(self, feat_f1, feat_c1, data, stride):
        win = gather_windows(feat_f1, data["b_ids"], data["j_ids"], stride, self.W)
        if self.cat_c_feat:
            pick = feat_c1.view(feat_c1.shape[0], feat_c1.shape[1], -1)[data["b_ids"], :, data["j_ids"]]
            down = self.down_proj(pick)
            return self.merge_feat(torch.cat([down.unsqueeze(1).expand(-1, self.W ** 2, -1), win], dim=2))
        return self.proj(win)

    # ------------------------------------------------------------------ library path
    def _pack(self, device):
        lib = _lib.load()
        need = lib.nl_fine_proj_packed_bytes(self.in_channels_fine, self.out_channels)
        if need == 0:
            raise RuntimeError(f"FinePreprocess: channels {self.in_channels_fine} -> {self.out_channels} are not supported by the HIP kernel "
                               "(multiples of 32, 32..256)")

        def pack(ts):
            packed = torch.empty(need, dtype=torch.uint8, device=device)
            st = _lib.stream(device)
            _lib.check(lib.nl_fine_pack_proj(self.in_channels_fine, self.out_channels, ts[0].data_ptr(), ts[1].data_ptr(), packed.data_ptr(), need, st),
                       "nl_fine_pack_proj")
            return packed
        return self._cached(device, [self.proj.weight, self.proj.bias], pack)

    def _pack_train(self, device):
        """The training image (proj.weight^T, nl_fine_pack_proj_train), cached like the inference image."""
        lib = _lib.load()
        need = lib.nl_fine_proj_train_bytes(self.in_channels_fine, self.out_channels)

        def pack(ts):
            packed = torch.empty(need, dtype=torch.uint8, device=device)
            st = _lib.stream(device)
            _lib.check(lib.nl_fine_pack_proj_train(self.in_channels_fine, self.out_channels, ts[0].data_ptr(), packed.data_ptr(), need, st), "nl_fine_pack_proj_train")
            return packed
        return self._train_cache._cached(device, [self.proj.weight], pack)

    def train_rows_precision(self):
        """The precision of the window rows of a TRAINING forward.  Every gradient is taken at these rows, and 2^-17 of a row's scale (split-bf16) is enough to
        move the heat-map by 1e-4 (the softmax multiplies it by the logit's size) and to put a ReLU unit that lies near its kink on the other side, so the
        parity mode computes them in exact fp32 (119 us instead of 79 us at the shipped size); the backward products stay three-term split-bf16."""
        return "fp32" if self.precision == "bf16x3" else self.precision

    def _windows_call(self, feat_f1, b_ids, j_ids, stride, precision=None, check_ids=True):
        """nl_fine_windows: (out (M, 49, out_channels), the NHWC map it read, b, j as int64 device tensors, the packed image).
        check_ids=False (internal: Matcher.forward_padded, whose ids come from the library's own selection over this map's grid, checked there against the number
        of coarse cells) skips the host range check and with it the read-back."""
        require_device("FinePreprocess", feat_f1)
        if self.W != 7:
            raise RuntimeError("FinePreprocess: the HIP kernel is built for fine_window_size 7")
        if feat_f1.dim() != 4 or feat_f1.shape[1] != self.in_channels_fine:
            raise ValueError(f"FinePreprocess: feat_f1 must be (B, {self.in_channels_fine}, Hf, Wf)")
        dev = feat_f1.device
        B, _, Hf, Wf = feat_f1.shape
        nhwc = feat_f1.detach().to(torch.float32).permute(0, 2, 3, 1)
        if not nhwc.is_contiguous():
            nhwc = nhwc.contiguous()   # the one NHWC copy of a plain NCHW input
        b = b_ids.to(device=dev, dtype=torch.int64).contiguous()
        j = j_ids.to(device=dev, dtype=torch.int64).contiguous()
        M = j.shape[0]
        if stride < 1 or b.shape[0] != M:
            _lib.check(_lib.NL_ERR_BAD_ARG, "nl_fine_windows (stride / id shapes)")
        L = ((Hf - 1) // stride + 1) * ((Wf - 1) // stride + 1)
        # entry points validate from the host (the kernel only keeps a bad id from reading foreign memory)
        if check_ids and M and bool(((j < 0) | (j >= L) | (b < 0) | (b >= B)).any()):   # one reduction, one read-back
            _lib.check(_lib.NL_ERR_BAD_ARG, f"nl_fine_windows (j_ids outside [0, {L}) or b_ids outside [0, {B}))")
        lib = _lib.load()
        with torch.cuda.device(dev):
            packed = self._pack(dev)
            out = torch.empty((M, 49, self.out_channels), dtype=torch.float32, device=dev)
            st = _lib.stream(dev)
            _lib.check(lib.nl_fine_windows(packed.data_ptr(), self.in_channels_fine, self.out_channels, _lib.PRECISIONS[precision or self.precision],
                                           nhwc.data_ptr(), B, Hf, Wf, b.data_ptr(), j.data_ptr(), M, stride, out.data_ptr(), st), "nl_fine_windows")
        return out, nhwc, b, j, packed

    def windows(self, feat_f1, b_ids, j_ids, stride):
        """The library call: (M, 49, out_channels) from feat_f1 (B, C, Hf, Wf) — a permuted view of an NHWC tensor is used as it is."""
        return self._windows_call(feat_f1, b_ids, j_ids, int(stride))[0]

    def forward(self, feat_f1, feat_c1, data):
        stride = data["stride_coarse"] // data["stride_fine"]
        if len(data["j_ids"]) == 0:
            return torch.empty(0, self.W ** 2, self.out_channels, device=feat_f1.device)
        if self.cat_c_feat or self.training or (torch.is_grad_enabled() and feat_f1.requires_grad):
            if self.hip_training and feat_f1.is_cuda and not self.cat_c_feat and len(data["j_ids"]) <= _lib.FINE_BACKWARD_MAX_M:
                # eval mode differentiates with respect to the map only: detached parameters are NULL gradient pointers in the backward call
                w, b = (self.proj.weight, self.proj.bias) if self.training else (self.proj.weight.detach(), self.proj.bias.detach())
                return _FineWindowsFn.apply(self, data["b_ids"], data["j_ids"], int(stride), feat_f1, w, b)
            return self._eager(feat_f1, feat_c1, data, stride)
        return self.windows(feat_f1, data["b_ids"], data["j_ids"], stride)


class _FineMatchFn(torch.autograd.Function):
    """(feat_f0, feat_f1, six parameters) -> (expec_f, mkps2d_f): nl_fine_match with the heat-map kept, and nl_fine_match_backward.  Parameters that do not
    require grad get a NULL gradient pointer.  The backward pass is not differentiable: a second-order backward raises."""

    @staticmethod
    def forward(ctx, mod, mkps2d_c, feat_f0, feat_f1, *params):
        expec, kf, heat, f0, f1, packed = mod._match_call(feat_f0, feat_f1, mkps2d_c, True)
        ctx.mod = mod
        # the images of the weights this forward ran on: a parameter changed in place before backward() must not meet the saved heat-map
        ctx.packed, ctx.tpacked = packed, pack_matcher_mlp_train("FineMatching", mod, f0.device) if any(ctx.needs_input_grad) else None
        ctx.in_dtypes = (feat_f0.dtype, feat_f1.dtype)
        ctx.save_for_backward(f0, f1, heat)
        ctx.mark_non_differentiable(kf)
        return expec, kf

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_expec, _g_kf):
        mod = ctx.mod
        f0, f1, heat = ctx.saved_tensors
        lib = _lib.load()
        dev = f0.device
        M, Cf = f0.shape[0], mod.feat_dim
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.nl_fine_match_backward_workspace_bytes(M, Cf), dev, "FineMatching: shape not supported by the training kernels")
            ge = g_expec.detach().to(torch.float32).contiguous()
            g_f0 = torch.empty_like(f0) if need[2] else None
            g_f1 = torch.empty_like(f1) if need[3] else None
            params, g_params = matcher_mlp_grad_buffers(mod, need[4:], dev)
            st = _lib.stream(dev)
            ptr = _lib.ptr
            _lib.check(lib.nl_fine_match_backward(ctx.packed.data_ptr(), ctx.tpacked.data_ptr(), Cf, _lib.PRECISIONS[mod.precision], f0.data_ptr(), f1.data_ptr(), M,
                                                  heat.data_ptr(), ge.data_ptr(), ptr(g_f0), ptr(g_f1), *[ptr(g) for g in g_params], ws.data_ptr(), ws.numel(), st),
                       "nl_fine_match_backward")
        return (None, None, None if g_f0 is None else g_f0.to(ctx.in_dtypes[0]), None if g_f1 is None else g_f1.to(ctx.in_dtypes[1]),
                *matcher_mlp_grads_out(params, g_params))


class _FineWindowsFn(torch.autograd.Function):
    """(feat_f1, proj.weight, proj.bias) -> the window rows (M, 49, Cout): nl_fine_windows and nl_fine_windows_backward.  The map's gradient comes back as a
    permuted view of an NHWC tensor, the layout the forward reads: an NHWC map costs no layout copy either way."""

    @staticmethod
    def forward(ctx, mod, b_ids, j_ids, stride, feat_f1, weight, bias):
        out, nhwc, b, j, packed = mod._windows_call(feat_f1, b_ids, j_ids, stride, mod.train_rows_precision())
        ctx.mod, ctx.stride, ctx.in_dtype = mod, stride, feat_f1.dtype
        ctx.packed, ctx.tpacked = packed, mod._pack_train(nhwc.device) if any(ctx.needs_input_grad) else None
        ctx.save_for_backward(nhwc, b, j)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        mod = ctx.mod
        nhwc, b, j = ctx.saved_tensors
        lib = _lib.load()
        dev = nhwc.device
        B, Hf, Wf, Cf = nhwc.shape
        Cout, M = mod.out_channels, j.shape[0]
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.nl_fine_windows_backward_workspace_bytes(Cf, Cout, B, Hf, Wf, ctx.stride, M), dev,
                                "FinePreprocess: shape not supported by the training kernels")
            go = g_out.detach().to(torch.float32).contiguous()
            g_map = torch.empty_like(nhwc) if need[4] else None
            g_w = torch.empty((Cout, Cf), dtype=torch.float32, device=dev) if need[5] else None
            g_b = torch.empty((Cout,), dtype=torch.float32, device=dev) if need[6] else None
            st = _lib.stream(dev)
            ptr = _lib.ptr
            _lib.check(lib.nl_fine_windows_backward(ctx.packed.data_ptr(), ctx.tpacked.data_ptr(), Cf, Cout, _lib.PRECISIONS[mod.precision], nhwc.data_ptr(), B, Hf, Wf,
                                                    b.data_ptr(), j.data_ptr(), M, ctx.stride, go.data_ptr(), ptr(g_w), ptr(g_b), ptr(g_map), ws.data_ptr(), ws.numel(),
                                                    st), "nl_fine_windows_backward")
        return (None, None, None, None, None if g_map is None else g_map.permute(0, 3, 1, 2).to(ctx.in_dtype),
                None if g_w is None else g_w.to(mod.proj.weight.dtype), None if g_b is None else g_b.to(mod.proj.bias.dtype))


class FineMatching(nn.Module, PackedCache):
    """`FineMatching(config)` ("FineMatching with s2d paradigm") with the reference's config keys and parameter names (`mlps.{0,2,4}.*`), so
    `matcher.fine_matcher.*` of a NeRF-Loc checkpoint loads with strict=True.  precision and hip_training as for FinePreprocess."""
    hip_training = True

    def __init__(self, config, precision: str = "bf16x3"):
        super().__init__()
        self._train_cache = new_train_cache()
        self.correct_thr = config["correct_thr"]
        self.loss_type = config["loss_type"]
        self.feat_dim = int(config["feat_dim"])
        self.mlps = nn.Sequential(nn.Linear(self.feat_dim, MATCHER_HIDDEN), nn.ReLU(inplace=True), nn.Linear(MATCHER_HIDDEN, MATCHER_HIDDEN), nn.ReLU(inplace=True),
                                  nn.Linear(MATCHER_HIDDEN, 1))
        self.precision = check_precision(precision)
        self._cache_init()

    # ------------------------------------------------------------------ library path
    def _pack(self, device):
        return pack_matcher_mlp("FineMatching", self, device)

    def _match_call(self, feat_f0, feat_f1, mkps2d_c, want_heatmap):
        """nl_fine_match: (expec_f, mkps2d_f, heatmap or None, the fp32 features it read, the packed image)."""
        require_device("FineMatching", feat_f0, feat_f1)
        M = feat_f0.shape[0]
        if feat_f0.dim() != 2 or feat_f0.shape[1] != self.feat_dim or tuple(feat_f1.shape) != (M, 49, self.feat_dim):
            raise ValueError(f"FineMatching: features must be (M, {self.feat_dim}) and (M, 49, {self.feat_dim})")
        dev = feat_f0.device
        lib = _lib.load()
        f0 = feat_f0.detach().to(torch.float32).contiguous()
        f1 = feat_f1.detach().to(torch.float32).contiguous()
        kc = mkps2d_c.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(kc.shape) != (M, 2):
            raise ValueError("FineMatching: mkps2d_c must be (M, 2)")
        with torch.cuda.device(dev):
            packed = self._pack(dev)
            expec = torch.empty((M, 3), dtype=torch.float32, device=dev)
            kf = torch.empty((M, 2), dtype=torch.float32, device=dev)
            heat = torch.empty((M, 49), dtype=torch.float32, device=dev) if want_heatmap else None
            st = _lib.stream(dev)
            _lib.check(lib.nl_fine_match(packed.data_ptr(), self.feat_dim, _lib.PRECISIONS[self.precision], f0.data_ptr(), f1.data_ptr(), M, kc.data_ptr(),
                                         expec.data_ptr(), kf.data_ptr(), _lib.ptr(heat), st), "nl_fine_match")
        return expec, kf, heat, f0, f1, packed

    def match(self, feat_f0, feat_f1, mkps2d_c, want_heatmap=False):
        """The library call: (expec_f (M, 3), mkps2d_f (M, 2), heatmap (M, 49) or None)."""
        return self._match_call(feat_f0, feat_f1, mkps2d_c, want_heatmap)[:3]

    # ------------------------------------------------------------------ forward
    def forward(self, feat_f0, feat_f1, data):
        M, WW, C = feat_f1.shape
        W = int(math.sqrt(WW))
        self.M, self.W, self.WW, self.C, self.scale = M, W, WW, C, data["stride_fine"]
        if M == 0:
            assert self.training is False, "M is always >0, when training, see coarse_matching.py"
            data.update({"expec_f": torch.empty(0, 3, device=feat_f0.device), "mkps2d_f": data["mkps2d_c"]})
            return
        if not (self.training or (torch.is_grad_enabled() and (feat_f0.requires_grad or feat_f1.requires_grad))):
            expec, kf, _ = self.match(feat_f0, feat_f1, data["mkps2d_c"])
            data.update({"expec_f": expec, "mkps2d_f": kf})
            return data
        if self.hip_training and feat_f0.is_cuda and feat_f1.is_cuda and M <= _lib.FINE_BACKWARD_MAX_M:
            # the library's training step: expec_f carries the graph, both losses below stay PyTorch on the (M, 3) tensor; eval mode differentiates with respect
            # to the features only (detached parameters are NULL gradient pointers in the backward call)
            params = [self.get_parameter(n) if self.training else self.get_parameter(n).detach() for n in MATCHER_MLP_PARAMS]
            expec, kf = _FineMatchFn.apply(self, data["mkps2d_c"], feat_f0, feat_f1, *params)
            data.update({"expec_f": expec})
            if self.training:
                data["fine_loss"] = self.get_loss(data["expec_f"], data["expec_f_gt"])
            data.update({"mkps2d_f": kf})
            return data
        # eager formulation (training / autograd)
        sim = self.mlps(torch.einsum("mc,mrc->mrc", feat_f0, feat_f1)).squeeze(-1)
        heatmap = torch.softmax((1.0 / C ** 0.5) * sim, dim=1)
        g = torch.linspace(-1, 1, W, device=heatmap.device, dtype=heatmap.dtype)
        grid = torch.stack([g[None, :].expand(W, W), g[:, None].expand(W, W)], dim=-1).reshape(1, WW, 2)   # x along the fast axis
        coords = (grid * heatmap[:, :, None]).sum(dim=1)
        var = torch.sum(grid ** 2 * heatmap[:, :, None], dim=1) - coords ** 2
        std = torch.sum(torch.sqrt(torch.clamp(var, min=1e-10)), -1)
        data.update({"expec_f": torch.cat([coords, std.unsqueeze(1)], -1)})
        if self.training:
            data["fine_loss"] = self.get_loss(data["expec_f"], data["expec_f_gt"])
        with torch.no_grad():
            data.update({"mkps2d_f": data["mkps2d_c"] + coords * (W // 2)})
        return data

    # ------------------------------------------------------------------ losses (fine_matching.py:155-207)
    def _correct_mask(self, expec_f_gt, weight=None):
        mask = torch.linalg.norm(expec_f_gt, ord=float("inf"), dim=1) < self.correct_thr
        if not mask.any():
            if not self.training:
                return None
            warnings.warn("FineMatching: no correct coarse match; assigning a false supervision to avoid a DDP deadlock")
            mask[0] = True
            if weight is not None:
                weight[0] = 0.0
        return mask

    def _compute_fine_loss_l2(self, expec_f, expec_f_gt):
        mask = self._correct_mask(expec_f_gt)
        if mask is None:
            return None
        return ((expec_f_gt[mask] - expec_f[mask, :2]) ** 2).sum(-1).mean()

    def _compute_fine_loss_l2_std(self, expec_f, expec_f_gt):
        inverse_std = 1.0 / torch.clamp(expec_f[:, 2], min=1e-10)
        weight = (inverse_std / torch.mean(inverse_std)).detach()   # the loss must not shrink by growing std
        mask = self._correct_mask(expec_f_gt, weight)
        if mask is None:
            return None
        offset_l2 = ((expec_f_gt[mask] - expec_f[mask, :2]) ** 2).sum(-1)
        return (offset_l2 * weight[mask]).mean()

    def get_loss(self, expec_f, expec_f_gt):
        if self.loss_type == "l2_with_std":
            return self._compute_fine_loss_l2_std(expec_f, expec_f_gt)
        if self.loss_type == "l2":
            return self._compute_fine_loss_l2(expec_f, expec_f_gt)
        raise NotImplementedError()
