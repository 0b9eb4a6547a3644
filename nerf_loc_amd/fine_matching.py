"""Drop-ins for the reference's fine matcher, `FinePreprocess` and `FineMatching` (models/matching/fine_matching.py:10-76 and :79-207, used by matcher.py:101-124).

Eval mode on a HIP device is one library call each (nl_fine_windows / nl_fine_match, csrc/fine.hip): the unfolded fine map, the M x 49 x C products and the hidden
activations of the reference's formulation are never materialised.  Training mode, an input that requires grad, or `fine_concat_coarse_feat=True` run the
reference's formulation in eager PyTorch (plumbing so that swapping the classes does not break a training script; there is no gradient kernel) — with the M windows
gathered directly instead of unfolding the whole map.  Eval mode on CPU tensors is refused: no CPU fallback.  kornia is not needed.
"""
from __future__ import annotations

import math
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._packing import MATCHER_HIDDEN, PackedCache, check_precision, pack_matcher_mlp, require_device

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
    """

    def __init__(self, config, precision: str = "bf16x3"):
        super().__init__()
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
            st = torch.cuda.current_stream(device).cuda_stream
            _lib.check(lib.nl_fine_pack_proj(self.in_channels_fine, self.out_channels, ts[0].data_ptr(), ts[1].data_ptr(), packed.data_ptr(), need, st),
                       "nl_fine_pack_proj")
            return packed
        return self._cached(device, [self.proj.weight, self.proj.bias], pack)

    def windows(self, feat_f1, b_ids, j_ids, stride):
        """The library call: (M, 49, out_channels) from feat_f1 (B, C, Hf, Wf) — a permuted view of an NHWC tensor is used as it is."""
        require_device("FinePreprocess", feat_f1)
        if self.W != 7:
            raise RuntimeError("FinePreprocess: the HIP kernel is built for fine_window_size 7")
        if feat_f1.dim() != 4 or feat_f1.shape[1] != self.in_channels_fine:
            raise ValueError(f"FinePreprocess: feat_f1 must be (B, {self.in_channels_fine}, Hf, Wf)")
        stride = int(stride)
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
        if M and bool(((j < 0) | (j >= L) | (b < 0) | (b >= B)).any()):   # one reduction, one read-back
            _lib.check(_lib.NL_ERR_BAD_ARG, f"nl_fine_windows (j_ids outside [0, {L}) or b_ids outside [0, {B}))")
        lib = _lib.load()
        with torch.cuda.device(dev):
            packed = self._pack(dev)
            out = torch.empty((M, 49, self.out_channels), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.nl_fine_windows(packed.data_ptr(), self.in_channels_fine, self.out_channels, _lib.PRECISIONS[self.precision], nhwc.data_ptr(),
                                           B, Hf, Wf, b.data_ptr(), j.data_ptr(), M, stride, out.data_ptr(), st), "nl_fine_windows")
        return out

    def forward(self, feat_f1, feat_c1, data):
        stride = data["stride_coarse"] // data["stride_fine"]
        if len(data["j_ids"]) == 0:
            return torch.empty(0, self.W ** 2, self.out_channels, device=feat_f1.device)
        if self.cat_c_feat or self.training or (torch.is_grad_enabled() and feat_f1.requires_grad):
            return self._eager(feat_f1, feat_c1, data, stride)
        return self.windows(feat_f1, data["b_ids"], data["j_ids"], stride)


class FineMatching(nn.Module, PackedCache):
    """`FineMatching(config)` ("FineMatching with s2d paradigm") with the reference's config keys and parameter names (`mlps.{0,2,4}.*`), so
    `matcher.fine_matcher.*` of a NeRF-Loc checkpoint loads with strict=True.  precision as for FinePreprocess."""

    def __init__(self, config, precision: str = "bf16x3"):
        super().__init__()
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

    def match(self, feat_f0, feat_f1, mkps2d_c, want_heatmap=False):
        """The library call: (expec_f (M, 3), mkps2d_f (M, 2), heatmap (M, 49) or None)."""
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
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.nl_fine_match(packed.data_ptr(), self.feat_dim, _lib.PRECISIONS[self.precision], f0.data_ptr(), f1.data_ptr(), M, kc.data_ptr(),
                                         expec.data_ptr(), kf.data_ptr(), heat.data_ptr() if want_heatmap else None, st), "nl_fine_match")
        return expec, kf, heat

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
