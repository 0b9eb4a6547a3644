"""Drop-in for the reference's `Matcher` (models/matcher.py:10-131): the localisation head as one object, built from this package's classes.

`Matcher(args, hidden_dim, in_channels_coarse, in_channels_fine, fine_matching=True)` has the reference's constructor, its 118 state-dict names (so `matcher.*` of a
NeRF-Loc checkpoint loads with strict=True) and its `forward(data)`, key for key.  Each stage takes whatever path its module takes: the library in eval mode on HIP
tensors, the modules' autograd Functions or eager paths in training mode or under autograd, and an error in eval mode on CPU tensors (no CPU fallback).

Two more entry points, eval mode on HIP tensors only, keep the NUMBER OF MATCHES on the device (libnerfloc_head.so, include/nerfloc_head.h):
  forward_padded(data, capacity)   the same stages with every per-match tensor of a fixed `capacity` rows, a device-side `num_matches`, no host read-back
  localize(data, K, thr, ...)      forward_padded, the fine key points scaled to pixels, and the pose solver with the count read on the device
                                   (nlh_pnp_ransac_counted): descriptors in, pose out, one linear chain of launches on the current stream, capturable in a graph
`forward` has exact shapes and therefore two host read-backs between the coarse and the fine stage (torch.nonzero, the id range check); the padded path computes
`capacity` fine rows whatever the count.  README.md gives the measured times of both and says which to prefer when.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _counted_lib, _head_lib, _lib
from ._packing import check_precision, require_device
from .fine_matching import FineMatching, FinePreprocess
from .matching import S2DMatching
from .pose import DEFAULT_HYPOTHESES, _intrinsics, _transforms
from .position_encoding import PositionEmbeddingSine, sine_table
from .transformer import SelfCrossTransformer


class Matcher(nn.Module):
    def __init__(self, args, hidden_dim, in_channels_coarse, in_channels_fine, fine_matching=True, precision: str = "bf16x3"):
        super().__init__()
        self.precision = check_precision(precision)
        self.hidden_dim = int(hidden_dim)
        self.coarse_transformer = SelfCrossTransformer(d_model=hidden_dim, dropout=0.1, nhead=8, dim_feedforward=512, num_encoder_layers=6, num_decoder_layers=6,
                                                       return_intermediate_dec=False, precision=precision)
        self.coarse_matcher = S2DMatching(hidden_dim, thr=0.2, precision=precision)
        self.fine_matching = fine_matching
        if fine_matching:
            self.pos_emd_2d_fn = PositionEmbeddingSine(hidden_dim // 2, normalize=True, sine_type="lin_sine")
            self.fine_window_size = 7
            self.fine_preprocess = FinePreprocess({"fine_concat_coarse_feat": False, "fine_window_size": self.fine_window_size, "in_channels_coarse": in_channels_coarse,
                                                   "in_channels_fine": in_channels_fine, "out_channels": hidden_dim}, precision=precision)
            self.fine_transformer = SelfCrossTransformer(d_model=hidden_dim, dropout=0.1, nhead=8, dim_feedforward=128, num_encoder_layers=6, num_decoder_layers=6,
                                                         return_intermediate_dec=False, precision=precision)
            self.fine_matcher = FineMatching({"feat_dim": hidden_dim, "correct_thr": 1.0, "loss_type": args.fine_matching_loss_type}, precision=precision)

    # ------------------------------------------------------------------ the reference's forward (matcher.py:63-131)
    def forward(self, data):
        desc_3d_trans_c, desc_2d_trans_c = self.coarse_transformer(data["desc_3d"][None, ...], data["pos_emd_3d"][None, ...], data["desc_2d_coarse"][None, ...],
                                                                   data["pos_emd_2d"][None, ...])
        data = self.coarse_matcher(desc_3d_trans_c[0], desc_2d_trans_c[0], data)
        i_ids, j_ids = data["i_ids"], data["j_ids"]
        data["b_ids"] = torch.zeros_like(i_ids)
        data.update({"mkps3d": data["kps3d"][i_ids], "mkps2d_c": data["kps2d"][j_ids], "pairs": [i_ids, j_ids]})
        if not self.fine_matching:
            return data
        if self.training:   # the ground-truth coarse pairs train the fine stage
            i_ids, j_ids = data["pairs_gt"][0], data["pairs_gt"][1]
            data.update({"b_ids": torch.zeros_like(i_ids), "i_ids": i_ids, "j_ids": j_ids, "mkps2d_c": data["kps2d"][j_ids], "mkps3d": data["kps3d"][i_ids]})
            data["expec_f_gt"] = (data["kps3d_proj_gt"][i_ids] - data["mkps2d_c"]) / (self.fine_window_size // 2)
        M = len(i_ids)
        if M == 0:   # no coarse match at all
            assert self.training is False, "M is always >0, when training"
            data.update({"expec_f": torch.empty(0, 3, device=data["mkps2d_c"].device), "mkps2d_f": data["mkps2d_c"]})
            return data
        W = self.fine_window_size
        feat_fine = data["feat_fine"].permute(0, 3, 1, 2)   # B, C, H, W
        feat_coarse = data["feat_coarse"].permute(0, 3, 1, 2) if data.get("feat_coarse") is not None else None   # read with fine_concat_coarse_feat alone
        matched_desc_3d = data["desc_3d_fine"][i_ids][:, None, :]
        matched_pos_emd_3d = data["pos_emd_3d"][i_ids][:, None, :]
        matched_desc_2d_fine = self.fine_preprocess(feat_fine, feat_coarse, data)   # M, WW, C
        matched_pos_emd_2d_fine = self.pos_emd_2d_fn(matched_desc_2d_fine[..., 0].view(M, W, W)).reshape(M, W * W, -1)   # the cached 7 x 7 table on a HIP device
        matched_desc_3d, matched_desc_2d_fine = self.fine_transformer(matched_desc_3d, matched_pos_emd_3d, matched_desc_2d_fine, matched_pos_emd_2d_fine)
        data = self.fine_matcher(matched_desc_3d[:, 0, :], matched_desc_2d_fine, data)
        if self.training:
            data["fine_err"] = torch.norm(data["expec_f_gt"] - data["expec_f"][:, :2], dim=-1).mean() * (W // 2) * data["stride_fine"]
        return data

    # ------------------------------------------------------------------ the padded path: the match count stays on the device
    def _padded_inputs(self, who, data):
        if self.training or not self.fine_matching:
            raise RuntimeError(f"Matcher.{who}: eval mode with fine matching only (training and fine_matching=False go through forward)")
        names = ("desc_3d", "pos_emd_3d", "desc_2d_coarse", "pos_emd_2d", "desc_3d_fine", "kps3d", "kps2d", "feat_fine")
        require_device(f"Matcher.{who}", *[data[n] for n in names])
        t = {n: data[n].detach().to(torch.float32).contiguous() for n in names[:7]}
        if torch.is_grad_enabled() and any(data[n].requires_grad for n in names):
            raise RuntimeError(f"Matcher.{who}: inputs that require grad go through forward (call under torch.no_grad())")
        return t

    @torch.no_grad()
    def forward_padded(self, data, capacity=None, num_points=None):
        """`forward` in eval mode with fixed shapes: i_ids, j_ids, b_ids, mkps3d, mkps2d_c, expec_f, mkps2d_f (and `pairs`) hold `capacity` rows, of which the first
        `num_matches` (a 0-d int32 DEVICE tensor) are forward's rows, in forward's order; `overflow` (0-d int32) is 1 when more rows matched than `capacity`, which
        then holds the first `capacity` of them.  capacity defaults to N: a 3-D point has at most one partner, so N cannot overflow.  Rows at and beyond
        num_matches are computed from zero descriptors and are finite; nothing may depend on them.  No host read-back; returns a new dict on top of `data`.
        num_points (default None: all N) is a 0-d int32 DEVICE tensor n: only the first n rows of the 3-D inputs (desc_3d, pos_emd_3d, desc_3d_fine, kps3d) exist
        (libnerfloc_counted.so).  The first num_matches rows are then forward's rows on those inputs cut to n rows, bit for bit; input rows at and beyond n must be
        finite and no valid row depends on them.  A host integer or a CPU tensor raises: it would hide a read-back or defeat graph replay."""
        if num_points is not None:
            _counted_lib.device_count(num_points, "Matcher.forward_padded")
        t = self._padded_inputs("forward_padded", data)
        N, Mc = t["desc_3d"].shape[0], t["desc_2d_coarse"].shape[0]
        cap = N if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError("Matcher.forward_padded: capacity must be at least 1")
        stride = int(data["stride_coarse"] // data["stride_fine"])
        feat_fine = data["feat_fine"].permute(0, 3, 1, 2)
        Bf, _, Hf, Wf = feat_fine.shape
        cells = ((Hf - 1) // max(stride, 1) + 1) * ((Wf - 1) // max(stride, 1) + 1)
        if tuple(t["kps2d"].shape) != (Mc, 2) or tuple(t["kps3d"].shape) != (N, 3) or Bf < 1 or stride < 1 or Mc > cells:
            # the selection's j_ids lie in [0, Mc): with Mc <= cells they are valid window ids, which is why the windows call needs no read-back here
            raise ValueError(f"Matcher.forward_padded: kps3d (N, 3), kps2d (Mc, 2) and at most one 2-D key point per coarse cell ({cells}) of feat_fine are required")
        if num_points is None:
            d3, d2 = self.coarse_transformer.transform(t["desc_3d"][None], t["pos_emd_3d"][None], t["desc_2d_coarse"][None], t["pos_emd_2d"][None])
            scores, match_j, _ = self.coarse_matcher.match(d3[0], d2[0])
        else:   # rows behind the count are no keys of the transformer and take no part in the selection's maxima; match_j is -1 there
            d3, d2 = self.coarse_transformer.transform(t["desc_3d"][None], t["pos_emd_3d"][None], t["desc_2d_coarse"][None], t["pos_emd_2d"][None], n0=num_points)
            scores, match_j, _ = self.coarse_matcher.match(d3[0], d2[0], n=num_points)
        sel = _head_lib.select_matches(match_j, cap, t["kps3d"], t["kps2d"], t["desc_3d_fine"], t["pos_emd_3d"])
        win = self.fine_preprocess._windows_call(feat_fine, sel["b_ids"], sel["j_ids"], stride, check_ids=False)[0]
        W = self.fine_window_size
        pos = sine_table(W, W, self.hidden_dim, win.device).view(1, W * W, self.hidden_dim).expand(cap, W * W, self.hidden_dim)
        f0, f1 = self.fine_transformer.transform(sel["out_a"][:, None, :], sel["out_b"][:, None, :], win, pos)
        expec, kf, _ = self.fine_matcher.match(f0[:, 0, :], f1, sel["mkps2d_c"])
        out = dict(data)
        out.update({"i_ids": sel["i_ids"], "j_ids": sel["j_ids"], "b_ids": sel["b_ids"], "score_matrix": scores, "mkps3d": sel["mkps3d"], "mkps2d_c": sel["mkps2d_c"],
                    "pairs": [sel["i_ids"], sel["j_ids"]], "expec_f": expec, "mkps2d_f": kf, "num_matches": sel["info"][_head_lib.INFO_COUNT],
                    "overflow": sel["info"][_head_lib.INFO_OVERFLOW], "match_info": sel["info"]})
        return out

    @torch.no_grad()
    def localize(self, data, K, thr, hypotheses: int = DEFAULT_HYPOTHESES, seed: int = 0, min_inliers: int = 4, capacity=None, num_points=None):
        """Descriptors in, pose out, without a host synchronisation: forward_padded, mkps2d_f * stride_fine, nlh_pnp_ransac_counted on the device count.
        K: (fx, fy, cx, cy) or a 3 x 3 matrix as numbers or a CPU tensor (a device tensor would cost a read-back), thr in pixels.  Returns DEVICE tensors: T_w2c,
        T_c2w (4 x 4 float64), inliers (capacity) bool — False at and beyond num_matches —, num_inliers, success, num_matches, overflow (0-d int32) and the padded
        match tensors of forward_padded.  The pose, mask and counts equal pose.absolute_pose on forward's matches with the same seed, bit for bit.  Fewer than
        four matches: the identity, success 0.  One linear chain on the current stream: capturable with torch.cuda.graph after one warm call.
        num_points: forward_padded's — with a 0-d int32 DEVICE tensor n the first num_matches rows, the pose, the mask and the counts equal `forward` followed by
        absolute_pose on the first n rows of the 3-D inputs, bit for bit (the second stage of cascade.localize_cascade); n == 0: the identity, success 0."""
        if torch.is_tensor(K) and K.is_cuda:
            raise ValueError("Matcher.localize: K must be numbers or a CPU tensor (a device tensor would synchronise)")
        fx, fy, cx, cy = _intrinsics(K)
        out = self.forward_padded(data, capacity, num_points)
        lib = _head_lib.load()
        p3 = out["mkps3d"]
        dev = p3.device
        cap = int(p3.shape[0])
        H = int(hypotheses)
        with torch.cuda.device(dev):
            p2 = (out["mkps2d_f"] * data["stride_fine"]).to(torch.float32).contiguous()
            ws = _lib.workspace(lib.nlh_pnp_workspace_bytes(cap, 1, H), dev, f"Matcher.localize: hypotheses must be a multiple of 64 in 64..65536, got {H}", ValueError)
            pose = torch.empty(1, 12, dtype=torch.float64, device=dev)
            mask = torch.empty(cap, dtype=torch.uint8, device=dev)
            info = torch.empty(1, 4, dtype=torch.int32, device=dev)
            offsets = (C.c_int32 * 2)(0, cap)
            intr = (C.c_double * 4)(fx, fy, cx, cy)
            thr_h = (C.c_double * 1)(float(thr))
            st = _lib.stream(dev)
            _lib.check(lib.nlh_pnp_ransac_counted(p2.data_ptr(), p3.data_ptr(), offsets, out["match_info"].data_ptr(), intr, thr_h, 1, H, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                  int(min_inliers), pose.data_ptr(), mask.data_ptr(), info.data_ptr(), None, ws.data_ptr(), ws.numel(), st),
                       "nlh_pnp_ransac_counted")
            T, Ti = _transforms(pose)
        res = {k: out[k] for k in ("i_ids", "j_ids", "b_ids", "mkps3d", "mkps2d_c", "mkps2d_f", "expec_f", "num_matches", "overflow", "score_matrix")}
        res.update({"T_w2c": T[0], "T_c2w": Ti[0], "inliers": mask.bool(), "num_inliers": info[0, 1], "success": info[0, 0], "best_candidate": info[0, 2],
                    "best_count": info[0, 3], "pts2d": p2})
        return res
