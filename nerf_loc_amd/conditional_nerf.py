"""Drop-in replacement for `nerf_loc.models.conditional_nerf.model.ConditionalNeRF` (reference model.py:29-713).

Same constructor (`ConditionalNeRF(args)` with the yacs field names of SURVEY.md §5), same public methods and return
dicts, same mutable caches (`support_neural_points`, `multiview_aggregator.vis_featmaps`) and the same state_dict
names/shapes, so `pl/model.py:33-41`-style checkpoint loading and
`nerf_pose_estimator.py:150,316,365,379,445,465` call sites work unchanged.

What runs where
  * everything per ray / per sample (rows a2-a20 of SURVEY.md §8) runs in libnerfloc_render.so (HIP, gfx950) through
    `HipRenderer`; there is NO PyTorch fallback for it — without the library or a GPU these methods raise.
  * ray generation (row a1: `get_rays`, `points_2d_to_rays`) is `nl_get_rays`.
  * per-frame setup (row a21): back-projection of the support views and DepthFusionNet's cross-view consistency input run in
    the library too (`frame_setup.py`: `nl_backproject_support`, `nl_cross_view_features`); the per-frame CNN itself
    (`DepthFusionNet.encode`, MIOpen convolutions), `confidence_mlp`, `keypoint_head` and the tiny descriptor projections stay on
    PyTorch-ROCm, like the 2-D backbone (north_star).
  * the two callers that differentiate THROUGH THE RENDERER — PoseOptimizer's `render_rays` under enable_grad and
    training (`compute_render_loss`, train-mode `render_rays` with `beta`) — run on the explicit gradient path of `diff_render.py`
    (fp32 autograd on the GPU around the HIP KNN), never on a silent fallback of the inference path; `query` / `render_image` refuse
    inputs that require grad.  The depth supervision of the per-frame CNN (`multiview_aggregator.compute_ref_depth_loss`) never
    touches the renderer and is implemented with autograd.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .depth_fusion import DepthFusionNet
from .frame_setup import backproject_support
from .frame_setup import get_rays as _hip_get_rays
from . import diff_render
from ._lib import GUARD_LOGIT_LIMIT as _GUARD_LOGIT_LIMIT
from ._lib import GUARD_DENSITY_LIMIT as _GUARD_DENSITY_LIMIT
from .renderer import HipRenderer


# ----------------------------------------------------------------------------- parameter containers (names = reference)
def _mlp(dims, act, last_act=None):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(act())
    if last_act is not None:
        layers.append(last_act())
    return nn.Sequential(*layers)


class _AddBias(nn.Module):
    def __init__(self, v):
        super().__init__()
        self.v = v

    def forward(self, x):
        return x + self.v


class MixtureLogisticsDistDecoder(nn.Module):
    """Parameter container for visibility_decoder.py:53-97 (the arithmetic runs in mvagg.hip / hier.hip)."""

    def __init__(self):
        super().__init__()
        self.mean_decoder = _mlp([32, 32, 32, 2], nn.ELU, nn.Softplus)
        self.var_decoder = nn.Sequential(*list(_mlp([32, 32, 32, 2], nn.ELU, nn.Softplus)), _AddBias(0.05))
        self.aw_decoder = _mlp([32, 32, 32, 1], nn.ELU, nn.Sigmoid)
        self.vis_decoder = _mlp([32, 32, 32, 1], nn.ELU, nn.Sigmoid)


class MultiviewFeatureAggregator(nn.Module):
    """multiview_aggregator.py:21-38: owns `depth_fusion` (PyTorch, per frame), `dist_decoder`, `out_fc` and the
    `vis_featmaps` cache the caller resets every frame (nerf_pose_estimator.py:289-290)."""

    def __init__(self, args, in_channels, out_channels, hidden_dim=64):
        super().__init__()
        self.args = args
        self.depth_fusion = DepthFusionNet(in_channels=in_channels)
        self._vis_gen = 0
        self.vis_featmaps = None
        self.dist_decoder = MixtureLogisticsDistDecoder()
        self.out_fc = nn.Sequential(nn.Linear((in_channels + 3) * 2 + 2 + 1, hidden_dim), nn.ELU(inplace=True),
                                    nn.Linear(hidden_dim, out_channels), nn.ELU(inplace=True))

    # `vis_featmaps` is a cache the CALLER resets by plain assignment (nerf_pose_estimator.py:290).  Every assignment bumps a
    # generation counter, which is what the HIP frame tables are keyed on (object ids / data pointers can be reused).
    @property
    def vis_featmaps(self):
        return self.__dict__.get("_vis_featmaps")

    @vis_featmaps.setter
    def vis_featmaps(self, v):
        self.__dict__["_vis_featmaps"] = v
        self.__dict__["_vis_gen"] = self.__dict__.get("_vis_gen", 0) + 1

    # ---- training-time depth supervision of the per-frame CNN (multiview_aggregator.py:39-61).  Everything here lives on the
    # PyTorch-ROCm side (DepthFusionNet + the 32-32-32-2 mean decoder): it is differentiable through autograd like the reference; the
    # only library call is the CNN's hand-made input (`nl_cross_view_features`), which has no parameters.
    def predict_ref_depths(self, intrinsics, extrinsics, images, featmaps, depths, depth_range, cnn_in=None):
        """-> (V, H/4, W/4) predicted depths of the support views.  `cnn_in` (V,12,H,W) optionally supplies DepthFusionNet's input
        (tests without a GPU); otherwise it comes from the HIP library."""
        vis = self.vis_featmaps
        if vis is None or (torch.is_grad_enabled() and not vis.requires_grad and any(p.requires_grad for p in self.depth_fusion.parameters())):
            vis = self.depth_fusion.encode(cnn_in) if cnn_in is not None else self.depth_fusion(images, featmaps, depths, intrinsics, extrinsics, depth_range)
            self.vis_featmaps = vis
        dr = depth_range.view(1, 2).repeat(vis.shape[0], 1).float()
        V, C, h, w = vis.shape
        mean = self.dist_decoder.mean_decoder(vis.view(V, C, -1).permute(0, 2, 1))      # (V, N, 2)   visibility_decoder.py:187-189
        near, far = dr[:, 0][:, None, None], dr[:, 1][:, None, None]                      # visibility_decoder.py:140-148
        near_inv, far_inv = -1 / near, -1 / far
        depth = -1 / (mean * (far_inv - near_inv) + near_inv)
        depth = depth.clamp(near.min(), far.max())
        return depth[:, :, 0].view(V, h, w)

    def compute_ref_depth_loss(self, intrinsics, extrinsics, images, featmaps, depths, depths_gt, depth_range, cnn_in=None):
        """multiview_aggregator.py:50-61: L2 between the inverse-normalised predicted and ground-truth support depths (valid pixels)."""
        import torch.nn.functional as F
        near, far = depth_range
        pred = self.predict_ref_depths(intrinsics, extrinsics, images, featmaps, depths, depth_range, cnn_in=cnn_in)
        V, h, w = pred.shape
        gt = F.interpolate(depths_gt.unsqueeze(1), size=(h, w)).view(V, -1)
        mask = gt > 0

        def inv_norm(d):   # losses.py:15-21
            near_inv, far_inv = -1 / near, -1 / far
            d = -1 / torch.clamp(d, min=1e-5)
            return torch.clamp((d - near_inv) / (far_inv - near_inv), min=0, max=1.0)
        return ((inv_norm(gt) - inv_norm(pred.view(V, -1)))[mask] ** 2).mean()


class _MHAParams(nn.Module):
    """ibrnet/ibrnet.py:72-87 parameter names."""

    def __init__(self, n_head, d_model, d_k, d_v):
        super().__init__()
        self.w_qs = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(d_model, n_head * d_v, bias=False)
        self.fc = nn.Linear(n_head * d_v, d_model, bias=False)
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)


class _RayUnetParams(nn.Module):
    """ray_unet.py:5-53 parameter names/shapes (Conv / ConvTranspose weights + LayerNorm([C,S]) affine)."""

    def __init__(self, W, S):
        super().__init__()

        def blk(conv, c, s):
            return nn.Sequential(conv, nn.LayerNorm([c, s]), nn.ELU(inplace=True))
        self.conv1 = blk(nn.Conv1d(W, 64, 3, 1, padding=1), 64, S)
        self.conv2 = blk(nn.Conv1d(64, 128, 3, 1, padding=1), 128, S // 2)
        self.conv3 = blk(nn.Conv1d(128, 128, 3, 1, padding=1), 128, S // 4)
        self.trans_conv3 = blk(nn.ConvTranspose1d(128, 128, 3, 2, padding=1, output_padding=1), 128, S // 4)
        self.trans_conv2 = blk(nn.ConvTranspose1d(256, 64, 3, 2, padding=1, output_padding=1), 64, S // 2)
        self.trans_conv1 = blk(nn.ConvTranspose1d(128, 32, 3, 2, padding=1, output_padding=1), 32, S)
        self.conv_out = blk(nn.Conv1d(W + 32, W, 3, 1, padding=1), W, S)


def get_rays(H, W, K, c2w):
    """conditional_nerf/utils.py:56-70 on the HIP library (`nl_get_rays`, row a1) -> (rays_o, rays_d), each (H,W,3)."""
    return _hip_get_rays(H, W, K, c2w)


class ConditionalNeRF(nn.Module):
    # `support_neural_points` is the second cache the caller resets per frame (nerf_pose_estimator.py:289): same generation
    # counter scheme as MultiviewFeatureAggregator.vis_featmaps.
    @property
    def support_neural_points(self):
        return self.__dict__.get("_support_neural_points")

    @support_neural_points.setter
    def support_neural_points(self, v):
        self.__dict__["_support_neural_points"] = v
        self.__dict__["_sp_gen"] = self.__dict__.get("_sp_gen", 0) + 1
        self.__dict__["_sp_from_hip"] = False   # set by _build_support_hip: tables this module built itself, without a graph

    # Precision guard (round 5; at the C-ABI since round 6).  The split-product modes carry 2^-16 (f16mx) / 2^-17 (bf16x3) per product where the reference's fp32
    # carries 2^-24.  On well-conditioned inputs that is 1-2.5e-5 / 8e-6 of the outputs; the one amplifier tools/scale_sweep.py found is the attention over a
    # sample's 8 neighbours: a logit error is (relative product error) x |logit|, and a softmax over nearly tied neighbours hands it on undamped.  The kernels of
    # the neural-point branch report the largest |logit| they scored, and the LIBRARY acts on it: every inference batch goes down with
    # NL_RENDER_PRECISION_GUARD (include/nerfloc_render.h, ABI 7) — after the batch it reads the indicator and, beyond the limit the current mode was validated
    # to, renders that batch again and keeps the frame in the next more exact mode (f16mx -> bf16x3 -> fp32).  EVERY batch of a frame is checked (round 5 checked
    # the first only: a chunked render_image could pass on a benign first chunk — ADVICE r5), a NaN logit counts as beyond every limit, and the staged kernels
    # of W = 32 / 64 report the indicator too.  Limits (NL_GUARD_LOGIT_LIMIT_*): the |logit| up to which the mode stayed within 1e-4 of the CPU oracle on every
    # scene of the sweep with margin (profiles/r5_scale_sweep.txt, MX-FP6 build: f16mx 5.1e-5 at |logit| 64, 7.2e-5 at 95, 9.3e-5 at 142, 1.7e-4 at 462 — the
    # limit is 50 since round 6, it was 100; bf16x3 4.2e-5 at 475 and 0.9-1.7e-4 at ~1000; the synthetic BASELINE scenes sit at 4-6).
    # The guard's second indicator is the largest density of the frame's batches (NL_GUARD_DENSITY_LIMIT_F16MX = 32; bf16x3 met the bar at every density measured and
    # has no such limit): behind a surface one or two samples carry a ray and the density head multiplies geo's error by its gain (DESIGN.md 2.3,
    # tests/test_gpu_surfaces.py).  nl_render_rays_multi does not take the flag (its lanes must not synchronise), so render_rays_frames over several data dicts
    # applies the same two limits on the host after the call: the logit from the frame's diagnostics, the density from the per-sample densities it asks for.
    # precision_guard=False switches it off; `guard_events` lists what it did.
    LOGIT_LIMIT = dict(_GUARD_LOGIT_LIMIT)
    DENSITY_LIMIT = dict(_GUARD_DENSITY_LIMIT)
    _SAFER = {"f16mx": "bf16x3", "bf16x3": "fp32", "bf16": "bf16x3"}

    def __init__(self, args, activation_func=None, precision: str = "f16mx", device: Optional[str] = None, precision_guard: bool = True,
                 hip_frame_cnn: bool = False, hip_frame_cnn_training: bool = False):
        super().__init__()
        self.args = copy.deepcopy(args)
        C, W = args.backbone2d_fpn_dim, args.model_3d_hidden_dim
        self.C, self.W = C, W
        self.S = args.render.N_samples + args.render.N_importance
        act = lambda: nn.LeakyReLU(inplace=True)  # noqa: E731
        xyz_dim, view_dim = 3 + 3 * 2 * args.multires, 3 + 3 * 2 * args.multires_views
        if args.i_embed != 0 or args.multires != 10 or args.multires_views != 4:
            raise ValueError("the HIP renderer is built for multires=10, multires_views=4, i_embed=0 (all shipped configs)")
        F_ = 3 + C
        self.ray_diff_fc = nn.Sequential(nn.Linear(4, 16), act(), nn.Linear(16, view_dim), act())
        self.multiview_aggregator = MultiviewFeatureAggregator(args, in_channels=C, out_channels=W)
        if hip_frame_cnn:   # the per-frame CNN through libnerfloc_cnn.so where no gradient is wanted (DepthFusionNet.encode); off by default
            self.multiview_aggregator.depth_fusion.hip_encode = True
        if hip_frame_cnn_training:   # its forward + backward through libnerfloc_cnn_train.so where the parameters want gradients; off by default
            self.multiview_aggregator.depth_fusion.hip_training = True
        self.confidence_mlp = nn.Sequential(nn.Linear(W, 64), act(), nn.Linear(64, 1), nn.Sigmoid())
        self.keypoint_head = nn.Sequential(nn.Linear(C, 1), nn.Sigmoid())
        self.base_mlp = nn.Sequential(nn.Linear(F_ + xyz_dim + view_dim, W), act(), nn.Linear(W, W), act(), nn.Linear(W, W), act())
        self.base_mlp_attn = _MHAParams(4, W, 32, 32)
        self.base_mlp_agg_weight = nn.Sequential(nn.Linear(W, W), act(), nn.Linear(W, 1))
        self.support_neural_points = None
        self.ray_unet = _RayUnetParams(W, self.S)
        self.sigma_mlp = nn.Sequential(nn.Linear(W, 1), nn.Softplus())
        if args.render.render_feature:
            self.feat_mlp = nn.Sequential(nn.Linear(W, W), act(), nn.Linear(W, C))
        self.rgb_blending_mlp = nn.Sequential(nn.Linear(W + F_ + 1 + 4, 32), act(), nn.Linear(32, 16), act(), nn.Linear(16, 1))
        if args.render.use_render_uncertainty:
            self.beta_mlp = nn.Sequential(nn.Linear(W, 1), nn.Softplus())
            self.beta_min = 0.1
        if args.use_scene_coord_memorization:
            def cd():
                return nn.Sequential(nn.Linear(xyz_dim, W), nn.ReLU(inplace=True), nn.Linear(W, W), nn.ReLU(inplace=True),
                                     nn.Linear(W, args.matcher_hidden_dim))
            self.coord_desc_mlp_coarse, self.coord_desc_mlp_fine = cd(), cd()
        self.proj_layer_3d_coarse = nn.Linear(W + F_, args.matcher_hidden_dim)
        self.proj_layer_3d_fine = nn.Linear(W + F_, args.matcher_hidden_dim)
        # ---- HIP side
        self._precision = precision
        self.precision_guard = bool(precision_guard)
        self.guard_events = []
        self._device = device
        self._renderers: Dict[str, HipRenderer] = {}
        self._frame_token: Dict[str, object] = {}
        self._weights_version = -1
        # training steps (compute_render_loss): the stages whose weight gradients the library computes run as HIP autograd nodes
        # (diff_render's stage nodes, given their parameter tensors); False = the all-eager fp32 graph
        self.hip_training = True

    # ------------------------------------------------------------------ HIP plumbing
    def _renderer(self, level: str) -> HipRenderer:
        dev = self._device or str(next(self.parameters()).device)
        if not dev.startswith("cuda"):
            raise RuntimeError("ConditionalNeRF's ray path runs only on a HIP device (no CPU fallback); move the module to cuda")
        r = self._renderers.get(level)
        if r is None:
            r = HipRenderer(self.W, self.C, self.S, self._precision, device=dev)
            self._renderers[level] = r
        ver = sum(p._version for p in self.parameters())
        stale = [rr for rr in self._renderers.values() if ver != self._weights_version or not rr._weights_loaded]
        if stale:   # (a renderer created later in a step packs for itself: the others' state — and the autograd nodes that hold them — stay untouched)
            sd = dict(self.state_dict())
            if "feat_mlp.0.weight" not in sd:   # render.render_feature=False (model.py:84-89): the head does not exist and is never evaluated
                z = next(self.parameters()).new_zeros
                sd.update({"feat_mlp.0.weight": z(self.W, self.W), "feat_mlp.0.bias": z(self.W), "feat_mlp.2.weight": z(self.C, self.W),
                           "feat_mlp.2.bias": z(self.C)})
            for rr in stale:
                rr.load_weights(sd)
            self._weights_version = ver
        return r

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._weights_version = -1
        return out

    def _depth_range(self, data):
        """(near, far) of data['depth_range'] as python floats.  On a device tensor that read is a synchronisation point: it is done once per tensor
        (identity + version), not once per render call of a refinement / training loop."""
        t = data["depth_range"]
        if not isinstance(t, torch.Tensor):
            return float(t[0][0]), float(t[0][1])
        # The cache holds the TENSOR (a strong reference: its storage cannot be handed to another tensor while the entry lives) and compares object
        # identity + version.  (address, version, shape) is not a key: the reference builds data['depth_range'] fresh every forward
        # (nerf_pose_estimator.py:265), always version 0 and shape (1, 2), and the allocator reuses the address — round 3 served stale ranges that way.
        c = self.__dict__.get("_dr_cache")
        if c is None or c[0] is not t or c[1] != t._version:
            v = t[0].detach().cpu().tolist()
            c = (t, t._version, float(v[0]), float(v[1]))
            self.__dict__["_dr_cache"] = c
        return c[2], c[3]

    def _ensure_frame(self, data, level: str) -> HipRenderer:
        """(Re)build the HIP per-frame tables when the caller reset the caches (nerf_pose_estimator.py:289-290)."""
        if self.support_neural_points is None:
            self.build_support_neural_points(data)
        r = self._renderer(level)
        sp = self.support_neural_points[level]
        feat = data["feat_fine_src"] if level == "fine" else data["feat_coarse_src"]
        near, far = self._depth_range(data)
        vis = self._vis_featmaps(data)   # (re)computes the cache first, so its generation is final below
        # generation counters of the two caller-reset caches + the identity of everything else the tables are built from
        token = (self._sp_gen, self.multiview_aggregator._vis_gen, data["topk_images"].data_ptr(), feat.data_ptr(),
                 data["topk_Ks"].data_ptr(), data["topk_poses"].data_ptr(), near, far, id(sp), id(vis))
        if self._frame_token.get(level) != token:
            r.set_frame(data["topk_images"], feat.detach(), vis.detach(), data["topk_Ks"], data["topk_poses"], near, far,
                        {k: sp[k].detach() for k in ("xyz", "feature", "confidence", "direction")})
            r.set_precision(self._precision)   # (the precision guard may have escalated the previous frame)
            self._frame_token[level] = token
        return r

    def _guarded(self, r: HipRenderer, render):
        """render(precision_guard) -> outputs of one inference batch.  With the guard on the batch goes down with NL_RENDER_PRECISION_GUARD: the library checks the
        conditioning indicator after EVERY batch and re-renders in a more exact mode where needed (see LOGIT_LIMIT); here the renderer's configured mode follows
        the frame's (so that the stage calls of the same frame — descriptor queries — run in it too) and the event is recorded."""
        if not self.precision_guard:
            return render(False)
        out = render(True)
        d = r.diagnostics()
        mode = d["guard_precision"]
        if mode is not None and mode != r.precision:
            self.guard_events.append({"logit_absmax": d["logit_absmax"], "density_max": d["density_max"], "from": r.precision, "to": mode})
            del self.guard_events[:-64]
            r.set_precision(mode)
        return out

    def _vis_featmaps(self, data, graph: bool = False):
        """The DepthFusionNet maps cache (multiview_aggregator.py:29,178).  graph=True (training): the maps must carry their graph to the
        CNN's parameters / the feature maps like the reference's do — recomputed once per frame when the cached tensor has none and
        something upstream can actually receive a gradient."""
        agg = self.multiview_aggregator
        if graph and agg.vis_featmaps is not None and not agg.vis_featmaps.requires_grad and \
                (data["feat_fine_src"].requires_grad or any(q.requires_grad for q in agg.depth_fusion.parameters())):
            agg.vis_featmaps = None
        if agg.vis_featmaps is None:
            with torch.set_grad_enabled(graph and torch.is_grad_enabled()):
                agg.vis_featmaps = agg.depth_fusion(data["topk_images"], data["feat_fine_src"].permute(0, 3, 1, 2), data["topk_depths"],
                                                    data["topk_Ks"], data["topk_poses"], data["depth_range"][0])
        return agg.vis_featmaps

    # ------------------------------------------------------------------ gradient-path plumbing (nerf_loc_amd/diff_render.py)
    def _graph_params(self, weights_graph: bool):
        """Parameter dict of the gradient path: the live parameters (their graph is kept) or detached constants."""
        if weights_graph:
            return {**dict(self.named_buffers()), **dict(self.named_parameters())}
        return {k: v.detach() for k, v in self.state_dict().items()}

    @staticmethod
    def _zero_grad_touch(p, *tensors):
        """0 x (sum of the tensors whose gradient through the library's training nodes is IDENTICALLY zero): `base_mlp_agg_weight.*` (a softmax over K
        identical rows, model.py:415) and — through the normalised neighbour weights times K identical rows (model.py:419-427) — the support confidences,
        i.e. `confidence_mlp`.  The reference's autograd leaves ~1e-10 of rounding noise there; the library propagates nothing, which would leave
        `.grad` None and make them "unused parameters" under DistributedDataParallel.  Adding this scalar to an output gives them exact zeros."""
        ts = [p[n] for n in ("base_mlp_agg_weight.0.weight", "base_mlp_agg_weight.0.bias", "base_mlp_agg_weight.2.weight", "base_mlp_agg_weight.2.bias") if n in p]
        ts += [t for t in tensors if isinstance(t, torch.Tensor)]
        ts = [t for t in ts if t.requires_grad]
        if not ts:
            return 0.0
        return sum(t.sum() for t in ts) * 0.0

    def _frame_dict(self, data, level: str, graph: bool):
        """`fr` of diff_render's functions for one level.  graph: per-frame caches with their graphs (training)."""
        fnear, ffar = self._depth_range(data)
        sp = self.support_neural_points[level]
        if not graph:
            sp = {k: sp[k].detach() for k in ("xyz", "feature", "confidence", "direction")}
        vis = self._vis_featmaps(data, graph)
        return {"topk_Ks": data["topk_Ks"], "topk_poses": data["topk_poses"], "topk_images": data["topk_images"],
                "feat_fine_src": data["feat_fine_src"] if level == "fine" else data["feat_coarse_src"],
                "vis_featmaps": vis if graph else vis.detach(), "near": fnear, "far": ffar, "support": sp}

    def _ensure_support(self, data):
        """The `support_neural_points is None` guard of every reference entry point (model.py:278,313,473), plus: tables cached by an
        earlier no_grad call are rebuilt with their graphs when a training step needs them."""
        if self.support_neural_points is None:
            return self.build_support_neural_points(data)
        if self.training and torch.is_grad_enabled() and self.__dict__.get("_sp_from_hip", False):
            self._build_support_graph(data)   # (tables the CALLER injected are never replaced)

    def _build_support_graph(self, data):
        """build_support_neural_points as the reference runs it in a training step (model.py:144-201 outside no_grad): both tables carry
        their graph — features gathered from the backbone's maps, fine confidence = confidence_mlp(aggregate at the points), coarse
        keypoint scores — and are cached for the whole frame, so query_coarse, query_fine and compute_render_loss of one step share one
        graph (and one DepthFusionNet pass) like the reference's module caches do."""
        p = self._graph_params(True)
        fnear, ffar = self._depth_range(data)
        fr = {"topk_Ks": data["topk_Ks"], "topk_poses": data["topk_poses"], "topk_images": data["topk_images"],
              "feat_fine_src": data["feat_fine_src"], "vis_featmaps": self._vis_featmaps(data, True), "near": fnear, "far": ffar}
        fine = diff_render.support_tables_diff(p, fr, data["topk_depths"], int(data["stride_fine"]))
        coarse = diff_render.coarse_support_diff(p, data["topk_images"], data["feat_coarse_src"], data["topk_depths"], data["topk_Ks"],
                                                 data["topk_poses"], int(data["stride_coarse"]))
        self.support_neural_points = {"coarse": coarse, "fine": fine}
        self._frame_token.clear()
        if len(coarse["xyz"]) == 0:
            print(f"Error: zero support_neural_points {data.get('scene')} : {data.get('filename')}")

    # ------------------------------------------------------------------ per-frame setup (a21)
    def backproject_support_frame(self, imgs, feats, depths, Ks, c2ws, stride=1):
        """model.py:203-265 on the HIP library (`nl_backproject_support`: count / scan / fill, reference row order) ->
        (feature (M,3+C), xyz world, xyz in view 0's camera, direction + depth)."""
        return backproject_support(imgs, feats, depths, Ks, c2ws, int(stride))

    def estimate_neural_points_confidence(self, points, data, level_feat):
        """model.py:137-142: confidence_mlp(multiview aggregate at the support points) — aggregate on HIP, MLP on torch."""
        r = self._renderers["fine"]
        mv, _, _, _ = r.mv_aggregate(points, data["pose"][:3, 3] if "pose" in data else torch.zeros(3), want_raw=False)
        return self.confidence_mlp(mv)

    def build_support_neural_points(self, data):
        """model.py:144-201.  Inference: HIP back-projection under no_grad.  In train() mode with autograd on the tables are built
        WITH their graphs (the reference builds them inside the training step's graph): `_build_support_graph`."""
        if self.training and torch.is_grad_enabled():
            return self._build_support_graph(data)
        with torch.no_grad():
            return self._build_support_hip(data)

    def _build_support_hip(self, data):
        d = data
        desc_c, pts_c, ndc_c, dir_c = self.backproject_support_frame(d["topk_images"], d["feat_coarse_src"], d["topk_depths"], d["topk_Ks"],
                                                                     d["topk_poses"], stride=d["stride_coarse"])
        desc_f, pts_f, ndc_f, dir_f = self.backproject_support_frame(d["topk_images"], d["feat_fine_src"], d["topk_depths"], d["topk_Ks"],
                                                                     d["topk_poses"], stride=d["stride_fine"])
        # the fine-level confidence needs the aggregator -> a frame with provisional confidence is set first
        fine = {"xyz": pts_f, "xyz_ndc": ndc_f, "feature": desc_f, "confidence": torch.ones_like(pts_f[:, :1]), "direction": dir_f}
        r = self._renderer("fine")
        near, far = self._depth_range(d)
        r.set_frame(d["topk_images"], d["feat_fine_src"], self._vis_featmaps(d), d["topk_Ks"], d["topk_poses"], near, far, fine)
        fine["confidence"] = self.estimate_neural_points_confidence(pts_f, d, None)
        self.support_neural_points = {
            "coarse": {"xyz": pts_c, "xyz_ndc": ndc_c, "feature": desc_c, "confidence": torch.ones_like(pts_c[:, :1]), "direction": dir_c,
                       "keypoint_score": self.keypoint_head(desc_c[:, 3:])},
            "fine": fine,
        }
        self._frame_token.clear()   # (the assignment above bumped the generation too) every level rebuilds its tables on next use
        self.__dict__["_sp_from_hip"] = True
        if len(pts_c) == 0:
            print(f"Error: zero support_neural_points {d.get('scene')} : {d.get('filename')}")

    # ------------------------------------------------------------------ descriptor queries (model.py:267-342)
    def sample_points_3d(self):
        sp = self.support_neural_points["coarse"]
        n = len(sp["xyz"])
        k = self.args.matching.fine_num_3d_keypoints
        idx = torch.multinomial(sp["keypoint_score"].squeeze(1), k, replacement=n < k)
        return sp["xyz"][idx], sp["xyz_ndc"][idx], idx

    def query(self, data, xyz, support_featmaps=None, support_neural_points=None, direction=None, K=8, embed_a=None, target_proj_mat=None):
        """model.py:344-436.  `support_featmaps` / `support_neural_points` select the level exactly like the reference's
        call sites do (fine: model.py:325-331,509-517; coarse: :296-302)."""
        self._ensure_support(data)
        level = "coarse" if (support_neural_points is not None and support_neural_points is self.support_neural_points.get("coarse")) else "fine"
        if self._query_wants_graph(data, level, xyz, direction):
            return self._query_grad(data, xyz, level, direction, K)
        with torch.no_grad():
            return self._query_hip(data, xyz, level, direction, K)

    def _query_wants_graph(self, data, level, xyz, direction) -> bool:
        """A descriptor query needs the gradient path whenever autograd could reach anything through it: train() mode (the matcher loss
        trains base_mlp / the attention / the aggregator / the 2-D backbone through 'feature_agg', nerf_pose_estimator.py:316-320,
        445-448, 465-468), trainable weights under enable_grad, or an input / feature map / support table that requires grad.  The HIP
        path returns detached tensors and is only taken when nothing can."""
        if not torch.is_grad_enabled():
            return False
        if self.training or any(q.requires_grad for q in self.parameters()):
            return True
        sp = self.support_neural_points[level]
        maps = data["feat_fine_src"] if level == "fine" else data["feat_coarse_src"]
        return self._wants_grad(xyz, direction, maps, data.get("feat_fine_src"), self.multiview_aggregator.vis_featmaps, sp["feature"], sp["confidence"])

    def _query_grad(self, data, xyz, level, direction, K):
        """model.py:344-436 on the gradient path (diff_render.query_diff: fp32 autograd on the GPU, exact KNN indices from the HIP
        library).  Weights keep their graph in train() mode or when they require grad; the per-frame caches keep theirs when they were
        built in a training step (`_build_support_graph`)."""
        weights_graph = self.training or any(q.requires_grad for q in self.parameters())
        fr = self._frame_dict(data, level, graph=True)
        r = self._ensure_frame(data, level)
        p = self._graph_params(weights_graph)
        sp = fr["support"]
        if self.hip_training and weights_graph and xyz.is_cuda and not xyz.requires_grad and (direction is None or not direction.requires_grad) \
                and len(sp["xyz"]) >= 1 and r.train_capable():
            # a training step: the aggregation and the neural-point branch as the library's training nodes (HIP forward; backward with the
            # gradients of their parameters, of the level's feature maps, of the DepthFusionNet maps and of the support features).  What the
            # matcher loss differentiates is 'feature_agg' (nerf_pose_estimator.py:316-320, 445-448, 465-468); 'weights' keeps its graph to the
            # confidences; the two raw multi-view entries are returned without one.
            xyz = xyz.detach().float().contiguous()
            dirs = None if direction is None else direction[:, :3].detach().float().contiguous()
            G, _ = diff_render.MvAggFn.apply(xyz, r, fr["feat_fine_src"], fr["vis_featmaps"], *[p[n] for n in diff_render.MV_PARAMS])
            fa = diff_render.PointBranchFn.apply(xyz, dirs, G, r, int(K), sp["feature"], *[p[n] for n in diff_render.POINT_PARAMS])
            with torch.no_grad():
                _, rgb_feat, vis_ang, _ = r.mv_aggregate(xyz, data["pose"][:3, 3] if "pose" in data else torch.zeros(3))
                d2, idx = r.knn(xyz, K)
            dist = d2.sqrt()
            conf = self._neighbour_confidence(sp, idx, K)
            w = (1.0 / torch.clamp(dist, min=1e-8)) * (1.0 / K) * conf
            w = w / torch.clamp(w.sum(1, keepdim=True), min=1e-8)
            fa = fa + self._zero_grad_touch(p)
            feature = (fa / torch.clamp(w.sum(1, keepdim=True).detach(), min=1e-20)).unsqueeze(1).expand(-1, K, -1)
            # (entries other than 'feature_agg' / 'weights' come back WITHOUT a graph on this path; callers that differentiate them use
            #  diff_render.query_diff through `hip_training = False`)
            return {"feature_agg": fa, "feature": feature, "weights": w, "multiview_feature": rgb_feat[:, :, :self.C + 3],
                    "multiview_visibility": vis_ang[:, :, :1]}
        idx = r.knn(xyz.detach(), K)[1].long()
        return diff_render.query_diff(p, fr, xyz, direction, idx)

    @staticmethod
    def _neighbour_confidence(sp, idx, K):
        """knn_gather(confidence, idx) as the reference's wrapper does it (knn_utils.py:211-220): with fewer than K support points the first M columns
        are the real neighbours and only the columns k >= M are zero-filled (all K columns were zeroed here)."""
        M = len(sp["xyz"])
        if M == 0:
            return torch.zeros(idx.shape, dtype=sp["confidence"].dtype, device=idx.device)
        conf = sp["confidence"].reshape(-1)[idx.long().clamp(0, M - 1)]
        if M < K:
            conf = conf.clone()
            conf[:, M:] = 0
        return conf

    def _query_hip(self, data, xyz, level, direction, K):
        r = self._ensure_frame(data, level)
        mv, rgb_feat, vis_ang, _ = r.mv_aggregate(xyz, data["pose"][:3, 3] if "pose" in data else torch.zeros(3))
        dirs = None if direction is None else direction[:, :3].contiguous()
        fa, d2, idx = r.point_mlp(xyz, dirs, mv, K=K)
        sp = self.support_neural_points[level]
        dist = d2.sqrt()
        conf = self._neighbour_confidence(sp, idx, K)
        w = (1.0 / torch.clamp(dist, min=1e-8)) * (1.0 / K) * conf
        w = w / torch.clamp(w.sum(1, keepdim=True), min=1e-8)
        scale = w.sum(1, keepdim=True)
        feature = (fa / torch.clamp(scale, min=1e-20)).unsqueeze(1).expand(-1, K, -1)   # identical for all K rows (see point.hip)
        return {"feature_agg": fa, "feature": feature, "weights": w, "multiview_feature": rgb_feat[:, :, :self.C + 3],
                "multiview_visibility": vis_ang[:, :, :1]}

    def _nearest_feature(self, level, points, data):
        r = self._ensure_frame(data, level)
        _, idx = r.knn(points.detach(), 1)
        return self.support_neural_points[level]["feature"][idx[:, 0].long()]

    def query_coarse(self, data, points=None, embed_a=None):
        self._ensure_support(data)
        if points is None:
            pts3d, pts3d_ndc, sidx = self.sample_points_3d()
            feat2d = self.support_neural_points["coarse"]["feature"][sidx]
        else:
            pts3d = points
            w2c = data["topk_poses"][0].inverse()
            pts3d_ndc = (torch.matmul(w2c[:3, :3], points.T) + w2c[:3, 3:]).T
            feat2d = self._nearest_feature("coarse", points, data)
        q = self.query(data, pts3d, support_neural_points=self.support_neural_points["coarse"], K=8, embed_a=embed_a)
        desc = self.proj_layer_3d_coarse(torch.cat([q["feature_agg"], feat2d], 1))
        if self.args.use_scene_coord_memorization:
            desc = desc + self.coord_desc_mlp_coarse(self._embed_xyz(pts3d))
        return desc, pts3d, pts3d_ndc

    def query_fine(self, data, points, embed_a=None):
        self._ensure_support(data)
        feat2d = self._nearest_feature("fine", points, data)
        q = self.query(data, points, support_neural_points=self.support_neural_points["fine"], K=1, embed_a=embed_a)
        desc = self.proj_layer_3d_fine(torch.cat([q["feature_agg"], feat2d], 1))
        if self.args.use_scene_coord_memorization:
            desc = desc + self.coord_desc_mlp_fine(self._embed_xyz(points))
        return desc, None, None

    @staticmethod
    def _embed_xyz(x, n=10):
        out = [x]
        for f in 2.0 ** torch.linspace(0.0, n - 1, n):
            out += [torch.sin(x * f), torch.cos(x * f)]
        return torch.cat(out, -1)

    # ------------------------------------------------------------------ rendering
    @staticmethod
    def _wants_grad(*tensors) -> bool:
        return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)

    def _refuse_autograd(self, what, *tensors):
        """The HIP kernels return detached tensors: entry points without a gradient path fail loudly instead of silently dropping
        the gradient (render_rays and points_2d_to_rays have one: nerf_loc_amd/diff_render.py)."""
        if self._wants_grad(*tensors):
            raise NotImplementedError(f"{what}: an input requires grad, but this entry point has no gradient path "
                                      "(SURVEY.md §8f-2); call it under torch.no_grad() or detach the inputs")

    def sample_depths(self, N_samples, near, far):
        """model.py:451-458 (tiny, host-side torch like the reference)."""
        t = torch.linspace(0, 1, N_samples, device=near.device)
        if not self.args.render.lindisp:
            return near * (1 - t) + far * t
        return 1 / (1 / near * (1 - t) + 1 / far * t)

    def render_rays(self, data, rays, u: Optional[torch.Tensor] = None):
        """model.py:472-600, eval mode.  `u` optionally fixes sample_pdf's uniform draws (reference: torch.rand)."""
        if self.training:   # model.py:587-592: the training render carries `beta` and its graph reaches the weights
            return self._render_rays_grad(data, rays, u, train=True)
        if self._wants_grad(rays.get("rays_o"), rays.get("rays_d"), rays.get("pose"), data.get("pose")):
            return self._render_rays_grad(data, rays, u)
        with torch.no_grad():
            return self._render_rays(data, rays, u)

    def _render_rays_grad(self, data, rays, u, train=False):
        """The two callers that differentiate through render_rays, on the eager path of nerf_loc_amd/diff_render.py (fp32 autograd on the
        GPU) with the exact KNN and the hierarchical depths from the HIP library:
        * pose_optimizer.py:131-160 (eval mode under torch.enable_grad()): gradients to rays_o / rays_d / data['pose']; the network
          weights are constants (PoseOptimizer optimises the pose only);
        * compute_render_loss (train mode): the parameters keep their graph, the per-frame caches are rebuilt WITH their graphs like
          the reference's (fine support table: features gathered from the feature maps, confidence_mlp on the aggregate;
          DepthFusionNet maps), `beta` is returned.
        Both are checked against the reference's autograd in tests/test_diff_render.py."""
        if train:
            # the per-frame caches with their graphs, built once per frame and shared with the descriptor queries of the same step
            self._ensure_support(data)
            p = self._graph_params(True)
            fr = self._frame_dict(data, "fine", graph=True)
        r = self._ensure_frame(data, "fine")   # the KNN grid over exactly these points (keyed on the caches' generation counters)
        near, far = rays["depth_range"]
        o, d = rays["rays_o"], rays["rays_d"]
        R, N = o.shape[0], self.args.render.N_samples
        z = self.sample_depths(N, near, far).expand(R, N).contiguous()
        depth_coarse = None
        if self.args.render.N_importance > 0 and train:
            # training: the coarse weights keep their graph (depth_coarse is supervised, losses.py:83-88); the resampled depths do not
            # (model.py:495 detaches the weights)
            if u is None:
                u = torch.rand(R, self.args.render.N_importance, device=o.device)
            zc = self.sample_depths(64, near, far).expand(R, 64).contiguous()
            wc = diff_render.coarse_weights_diff(p, fr, rays["pixel_coordinates"].to(o.dtype), rays["K"], rays["pose"], zc)
            depth_coarse = (wc * zc).sum(1)
            zf = diff_render.sample_pdf_diff(0.5 * (zc[:, :-1] + zc[:, 1:]), wc[:, 1:-1].detach(), u)
            z = torch.sort(torch.cat([z, zf], -1), -1)[0]
        elif self.args.render.N_importance > 0:   # the resampled depths carry no gradient in the reference either (model.py:495 detaches)
            with torch.no_grad():
                if u is None:
                    u = torch.rand(R, self.args.render.N_importance, device=o.device)
                z, depth_coarse, _ = r.hierarchical_depths(rays["pixel_coordinates"], rays["K"], rays["pose"].detach(), z, u, near=near, far=far,
                                                           lindisp=bool(self.args.render.lindisp))
        if not train:   # eval mode: the weights and the per-frame caches are constants (PoseOptimizer optimises the pose only)
            fr = self._frame_dict(data, "fine", graph=False)
            p = self._graph_params(False)
        out = diff_render.render_rays_diff(p, fr, o, d, z.to(o.dtype), data["pose"], lambda q: r.knn(q, 8)[1],
                                           white_bkgd=bool(data.get("white_bkgd", self.args.render.white_bkgd)),
                                           beta=train and bool(self.args.render.use_render_uncertainty),
                                           frozen_renderer=None if train else r,   # eval: weights + support table are constants -> HIP backward of the point branch
                                           train_renderer=r if train and self.hip_training and o.is_cuda and r.train_capable() else None)
        if train and self.hip_training and o.is_cuda and r.train_capable():
            out["rgb"] = out["rgb"] + self._zero_grad_touch(p, fr["support"]["confidence"])
        if not self.args.render.render_feature:
            out.pop("feat")
        if depth_coarse is not None:
            out["depth_coarse"] = depth_coarse
        return out

    def _render_rays_multi(self, datas, rays_list, us=None):
        """render_rays_frames for frames with DIFFERENT support sets (round 4; the reference resets its caches and loops: nerf_pose_estimator.py:289-290,
        model.py:615-639): `datas[i]` is the `data` dict of frame i, `rays_list[i]` its rays.  Every frame gets its own renderer (frame tables, workspace)
        from a pool; the per-frame setup runs frame by frame like the reference's, then ALL frames' rays go down in one library call
        (nl_render_rays_multi: one launch chain per frame on library-owned streams).  Returns one output dict per frame, bit-identical to
        `render_rays(datas[i], rays_list[i])`.  The module's caller-visible caches are left holding the LAST frame's tables."""
        from .renderer import render_rays_multi
        if len(datas) != len(rays_list):
            raise ValueError("one rays dict per data dict")
        base = self._renderer("fine")   # (packs the current weights if needed)
        pool = self.__dict__.setdefault("_multi_pool", [])
        while len(pool) < len(datas):
            pool.append(HipRenderer(self.W, self.C, self.S, self._precision, device=str(base.device)))
        ver = self._weights_version
        sd = None
        N = self.args.render.N_samples
        jobs, dcs = [], []
        for i, (data, rays) in enumerate(zip(datas, rays_list)):
            r = pool[i]
            if getattr(r, "_pool_weights_version", None) != ver or not r._weights_loaded:
                if sd is None:
                    sd = dict(self.state_dict())
                    if "feat_mlp.0.weight" not in sd:
                        z0 = next(self.parameters()).new_zeros
                        sd.update({"feat_mlp.0.weight": z0(self.W, self.W), "feat_mlp.0.bias": z0(self.W), "feat_mlp.2.weight": z0(self.C, self.W),
                                   "feat_mlp.2.bias": z0(self.C)})
                r.load_weights(sd)
                r._pool_weights_version = ver
            # the per-frame setup, frame by frame (the reference's cache reset + rebuild)
            self.support_neural_points = None
            self.multiview_aggregator.vis_featmaps = None
            self.build_support_neural_points(data)
            sp = self.support_neural_points["fine"]
            near, far = self._depth_range(data)
            vis = self._vis_featmaps(data)
            r.set_precision(self._precision)
            r.set_frame(data["topk_images"], data["feat_fine_src"].detach(), vis.detach(), data["topk_Ks"], data["topk_poses"], near, far,
                        {k: sp[k].detach() for k in ("xyz", "feature", "confidence", "direction")})
            rn, rf = rays["depth_range"]
            o, d = rays["rays_o"], rays["rays_d"]
            R = o.shape[0]
            z = self.sample_depths(N, rn, rf).expand(R, N).contiguous()
            if self.args.render.N_importance > 0:
                u = us[i] if us is not None else torch.rand(R, self.args.render.N_importance, device=o.device)
                z, dc, _ = r.hierarchical_depths(rays["pixel_coordinates"], rays["K"], rays["pose"], z, u, near=rn, far=rf, lindisp=bool(self.args.render.lindisp))
                dcs.append(dc)
            # the query centre is data['pose'] like render_rays' (model.py:472-480 reads the pose of `data`; `rays['pose']` only feeds the hierarchical branch)
            jobs.append((r, o, d, data["pose"][:3, 3].detach(), {"z_vals": z, "white_bkgd": bool(data.get("white_bkgd", self.args.render.white_bkgd)),
                                                                  "want_feat": bool(self.args.render.render_feature), "want_sigma": bool(self.precision_guard)}))
        self._frame_token = {}   # (the single-frame renderers' tables no longer describe the module's caches)
        outs = render_rays_multi(jobs)
        if self.precision_guard:   # the conditioning check of `_guarded`, per frame: a frame beyond its mode's validated range is rendered again in the safer mode
            for i, job in enumerate(jobs):
                r = job[0]
                amax = r.diagnostics()["logit_absmax"]
                dmax = float(outs[i].pop("sigma").max())   # (the library's own indicator needs the flag nl_render_rays_multi refuses; NaN propagates through max)
                mode = r.precision
                # (written so that a NaN is beyond every limit, as in the library)
                while (mode in self.LOGIT_LIMIT and not amax <= self.LOGIT_LIMIT[mode]) or (mode in self.DENSITY_LIMIT and not dmax <= self.DENSITY_LIMIT[mode]):
                    mode = self._SAFER[mode]
                if mode != r.precision:
                    self.guard_events.append({"logit_absmax": amax, "density_max": dmax, "from": r.precision, "to": mode, "frame": i})
                    del self.guard_events[:-64]
                    r.set_precision(mode)
                    dc = outs[i].get("depth_coarse")
                    outs[i] = r.render_rays(job[1], job[2], job[3], **{k: v for k, v in job[4].items() if k != "want_sigma"})
                    if dc is not None:
                        outs[i]["depth_coarse"] = dc
        for o_, dc in zip(outs, dcs):
            o_["depth_coarse"] = dc
        return outs

    def release_multi_pool(self) -> None:
        """Drop the per-frame renderers `render_rays_frames(list of data dicts)` keeps between calls (their frame tables and workspaces: gigabytes for large batches)."""
        self.__dict__.pop("_multi_pool", None)

    def _render_rays(self, data, rays, u):
        r = self._ensure_frame(data, "fine")
        near, far = rays["depth_range"]
        o, d = rays["rays_o"], rays["rays_d"]
        R = o.shape[0]
        N = self.args.render.N_samples
        z = self.sample_depths(N, near, far).expand(R, N).contiguous()
        depth_coarse = None
        if self.args.render.N_importance > 0:
            if u is None:
                u = torch.rand(R, self.args.render.N_importance, device=o.device)
            # the coarse depths use the RAYS' range like the base samples (model.py:489), not the frame's
            z, depth_coarse, _ = r.hierarchical_depths(rays["pixel_coordinates"], rays["K"], rays["pose"], z, u, near=near, far=far,
                                                       lindisp=bool(self.args.render.lindisp))
        # (`inference_graphs`: replay small batch shapes as HIP graphs, HipRenderer.render_rays(graph=True).  Off by default: measured on the MI355X box the
        # replay buys nothing — 256 rays of config 1: 0.391 ms eager, 0.387 ms replayed, and the static-buffer copies around it cost more than that;
        # the chain is bound by its kernels' own ramp and tail, not by the host's launches — DESIGN.md 5.20)
        out = self._guarded(r, lambda g: r.render_rays(o, d, data["pose"][:3, 3], z_vals=z, white_bkgd=bool(data.get("white_bkgd", self.args.render.white_bkgd)),
                                                       want_feat=bool(self.args.render.render_feature), graph=bool(getattr(self, "inference_graphs", False)),
                                                       precision_guard=g))
        if depth_coarse is not None:
            out["depth_coarse"] = depth_coarse
        return out

    @torch.no_grad()
    def render_rays_frames(self, data, rays_list, us=None):
        """Several query frames per launch (no counterpart in the reference, which calls render_rays once per pose):
        `rays_list` holds one `rays` dict per query pose (as points_2d_to_rays / sample_rays return them, plus 'depth_range'), all
        against the support frame of `data`.  The query camera centre is the only per-query-frame quantity the ray path reads
        (ibrnet.py:144-167), so the rays go down in ONE library call with per-ray centres (nl_render_opts.ray_centers) and the launch chain
        is paid once — what matters for PoseOptimizer-sized batches (config 2, 512 rays: 1.65 ms alone, 1.30 ms per frame in a batch of
        eight; tools/multi_frame_bench.py).
        Returns one output dict per frame, identical to render_rays(data_with_that_pose, rays)."""
        if self.training:
            raise NotImplementedError("render_rays_frames is an inference entry point")
        if isinstance(data, (list, tuple)):
            return self._render_rays_multi(list(data), rays_list, us)
        r = self._ensure_frame(data, "fine")
        N = self.args.render.N_samples
        os_, ds_, zs, cs, dcs, counts = [], [], [], [], [], []
        for i, rays in enumerate(rays_list):
            near, far = rays["depth_range"]
            o, d = rays["rays_o"], rays["rays_d"]
            R = o.shape[0]
            z = self.sample_depths(N, near, far).expand(R, N).contiguous()
            if self.args.render.N_importance > 0:
                u = us[i] if us is not None else torch.rand(R, self.args.render.N_importance, device=o.device)
                z, dc, _ = r.hierarchical_depths(rays["pixel_coordinates"], rays["K"], rays["pose"], z, u, near=near, far=far,
                                                 lindisp=bool(self.args.render.lindisp))
                dcs.append(dc)
            os_.append(o); ds_.append(d); zs.append(z); counts.append(R)
            cs.append(rays["pose"][:3, 3].detach().to(o.device).expand(R, 3))
        O_, D_, C_, Z_ = torch.cat(os_), torch.cat(ds_), torch.cat(cs).contiguous(), torch.cat(zs)
        out = self._guarded(r, lambda g: r.render_rays(O_, D_, C_, z_vals=Z_, white_bkgd=bool(data.get("white_bkgd", self.args.render.white_bkgd)),
                                                       want_feat=bool(self.args.render.render_feature), precision_guard=g))
        outs = [dict(zip(out.keys(), parts)) for parts in zip(*(torch.split(v, counts) for v in out.values()))]
        for o_, dc in zip(outs, dcs):
            o_["depth_coarse"] = dc
        return outs

    def render_image(self, data):
        """model.py:602-639."""
        self._refuse_autograd("render_image", data.get("pose"), data.get("K"))
        with torch.no_grad():
            return self._render_image(data)

    def _render_image(self, data):
        H, W, K, pose = data["H"], data["W"], data["K"], data["pose"]
        o, d = get_rays(H, W, K, pose)
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        uu, vv = torch.meshgrid(torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H), indexing="ij")
        pix = torch.stack([uu.t().reshape(-1), vv.t().reshape(-1)], 1).to(K.device)
        # The reference loops over `render.chunk` rays to bound its activation memory (model.py:615-633); here the library bounds it
        # itself (nl_render_rays walks the batch in pieces of <= 2^20 samples inside one call), and rays are independent, so the
        # whole image goes down in one call: same result, no per-chunk host work.
        ret = self.render_rays(data, {"pixel_coordinates": pix, "K": K, "pose": pose, "H": H, "W": W, "rays_o": o, "rays_d": d,
                                      "depth_range": data["depth_range"][0]})
        out = {k: v.view(H, W, -1) for k, v in ret.items()}
        if "target_mask" in data:
            out["rgb"] = out["rgb"] * data["target_mask"][:, :, None].float()
        return out

    def render_image_sharded(self, data, dist):
        """render_image with the image's rays sharded over the ranks of an initialised process group and ONE all-gather of the per-ray outputs
        (nerf_loc_amd/sharding.py; no counterpart in the reference, whose render_image walks `render.chunk` pieces on one device: model.py:615-633).
        Every rank gets the whole image, bit-identical to render_image(data)."""
        from .sharding import render_image_sharded
        self._refuse_autograd("render_image_sharded", data.get("pose"), data.get("K"))
        return render_image_sharded(self, data, dist)

    def compute_render_loss(self, data):
        """model.py:641-685 (+ losses.py:23-93): one training step's render loss and PSNR on the gradient path (`_render_rays_grad`)."""
        if "sample_coords" in data:
            rays = self.points_2d_to_rays(data["sample_coords"], data["H"], data["W"], data["K"], data["pose"])
        else:
            rays = self.sample_rays(self.args.render.N_rand, data["H"], data["W"], data["K"], data["pose"], data.get("target_mask", None))
        uv = rays["pixel_coordinates"].long()
        targets = {"rgb": data["img"].permute(1, 2, 0)[uv[:, 1], uv[:, 0]]}
        rays["depth_range"] = data["depth_range"][0]
        preds = self.render_rays(data, rays)
        mask = preds["mask"]
        if self.args.use_depth_supervision:
            targets.update({"depth_range": data["depth_range"][0], "depth": data["depth"][uv[:, 1], uv[:, 0]]})
        if self.args.render.render_feature:
            fmap = F.interpolate(data["feat_pyramid"]["layer1"], size=(data["H"], data["W"]), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
            targets["feat"] = fmap[0, uv[:, 1], uv[:, 0]]
        if "target_mask" in data:
            mask = mask & data["target_mask"][uv[:, 1], uv[:, 0]]
            targets["mask"] = mask
        loss = diff_render.rendering_loss(preds, targets, use_depth=bool(self.args.use_depth_supervision))
        return loss, diff_render.masked_psnr(preds["rgb"], targets["rgb"], mask)

    def points_2d_to_rays(self, pts2d, H, W, K, pose):
        """model.py:687-700."""
        if self._wants_grad(pose, K):   # differentiable w.r.t. the pose (pose_optimizer.py:136)
            o, d = diff_render.rays_from_pose(pts2d, K, pose)
        else:
            o, d = _hip_get_rays(H, W, K, pose, uv=pts2d)   # only the requested pixels (the reference builds the whole grid and indexes it)
        return {"pose": pose, "K": K, "H": H, "W": W, "pixel_coordinates": pts2d, "rays_o": o, "rays_d": d}

    def sample_rays(self, n_rays, H, W, K, pose, mask=None):
        """model.py:702-713."""
        u, v = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="ij")
        pts = torch.stack([u.reshape(-1).float(), v.reshape(-1).float()], 1)
        if mask is not None:
            pts = pts[mask[pts[:, 1].long(), pts[:, 0].long()].bool().cpu()]
        idx = np.random.choice(len(pts), n_rays, replace=False)
        return self.points_2d_to_rays(pts[idx].to(K.device), H, W, K, pose)
