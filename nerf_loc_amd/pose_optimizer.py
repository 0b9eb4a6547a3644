"""PoseOptimizer (nerf_loc/models/pose_optimizer.py) on the HIP libraries: render-and-compare refinement of camera poses against one query frame.

`PoseOptimizer(args, nerf_renderer, ...)(pose, data, ...)` keeps the reference's signature, `data` keys and return value.  `refine` is the batched form underneath:
(B, 4, 4) poses on the device — `Matcher.localize`'s fp64 `T_c2w[None]` as it lies — go down as one B x Rp ray batch with per-ray centres, and the results come
back as device tensors without a host synchronisation.

The library loop (`hip_loop`): libnerfloc_refine.so's kernels around the renderer's keep / kept pair, on the static buffers of `renderer.GraphedKeep` — rays are
written where the pair reads them, outputs and gradients are read where it leaves them.  After one warm step a step is ONE captured graph,
  nlr_pose_rays -> nl_render_rays_forward_keep -> nlr_loss -> nl_render_rays_backward_kept -> nlr_step,
replayed max_steps - 1 times; the Adam state, the step counter, the NaN latch and the reference's "discard" rule live in device memory.  The graph and its static
buffers are kept per (frame, B, Rp, target, lr): a second refinement of the same shape against the same frame captures nothing.

The eager formulation is the reference's loop on the module's public calls (points_2d_to_rays, render_rays under enable_grad, torch.optim.Adam) with
`nerf_loc_amd.se3`.  It runs, chosen per call, when `hip_loop` is off, when render.N_importance > 0 (the reference redraws its samples every step), when the batch
does not fit diff_render.KEEP_BYTES, when diff_render.USE_GRAPHS is off, or while the renderer's keep buffers of the shape are held by a forward pass that still
waits for its backward; it returns the same keys.  CPU tensors raise: the renderer has no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import _refine_lib as RL
from . import diff_render
from .se3 import se3_exp_map, se3_log_map

BETAS, ADAM_EPS = (0.9, 0.999), 1e-8   # pose_optimizer.py:77 and torch.optim.Adam's default


class _Plan:
    """The static buffers of one refinement shape and the captured step that replays on them."""

    def __init__(self, key, gk, B, Rp, C, dev):
        self.key, self.gk = key, gk   # (holding gk keeps its identity, which is part of the key, from being reused)
        self.state = RL.new_state(B, dev)
        self.K = torch.empty((3, 3), dtype=torch.float32, device=dev)
        self.uv = torch.empty((Rp, 2), dtype=torch.float32, device=dev)
        self.target = torch.empty((Rp, C), dtype=torch.float32, device=dev)
        self.row_loss = torch.empty(B * Rp, dtype=torch.float64, device=dev)
        self.pose32 = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        self.graph = None
        self.stream = torch.cuda.Stream(device=dev)


class PoseOptimizer(object):
    hip_loop = True    # the library loop; False: the eager formulation (settable per instance)
    capture = True     # the library loop replays its step as one HIP graph after a warm step; False: every step is issued call by call (same bits)

    def __init__(self, args, nerf_renderer, debug=False, sampling='random', use_feat=True, num_rays=512):
        self.args = args
        self.sampling = sampling
        self.nerf_renderer = nerf_renderer
        self.debug = debug
        self.use_feat = use_feat
        self.num_rays = int(num_rays)
        self._plan = None
        if sampling == 'interest_region':
            raise NotImplementedError("sampling='interest_region' needs the reference's SuperPoint module and weights, which do not exist here")
        if sampling not in ('grid', 'random'):
            raise NotImplementedError(sampling)

    # ------------------------------------------------------------------ the reference's entry point
    def __call__(self, pose, data, max_steps=100, lr=0.001, scale=0.25, num_rays=None):
        dev = data['img'].device
        if not torch.is_tensor(pose):
            pose = torch.tensor(np.asarray(pose)).to(dev).float()
        if pose.shape == (3, 4):
            pose = torch.cat([pose, torch.tensor([0, 0, 0, 1], dtype=pose.dtype, device=pose.device).view(1, 4)])
        out = self.refine(pose.to(dev)[None].contiguous(), data, max_steps=max_steps, lr=lr, scale=scale, num_rays=num_rays)
        return out["T_c2w32"][0]

    # ------------------------------------------------------------------ pixels (pose_optimizer.py:108-127)
    def sample_pixels(self, data, H, W, num_rays=None):
        """(Rp, 2) int64 (x, y) on the CPU, as the reference draws them: 'grid' every tenth pixel, 'random' `num_rays` of the frame's (or data['target_mask']'s)
        pixels through np.random.choice, so np.random.seed governs it."""
        if self.sampling == 'grid':
            v, u = torch.meshgrid(torch.arange(0, H, 10), torch.arange(0, W, 10), indexing="ij")
            return torch.stack([u.reshape(-1), v.reshape(-1)], 1)
        if 'target_mask' in data:
            v, u = torch.where(data['target_mask'].cpu() > 0)
            uv = torch.stack([u, v], 1)
        else:
            u, v = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="ij")
            uv = torch.stack([u.reshape(-1), v.reshape(-1)], 1)
        n = self.num_rays if num_rays is None else int(num_rays)
        return uv[np.random.choice(len(uv), n, replace=False)]

    # ------------------------------------------------------------------ the batched form
    def refine(self, poses, data, *, uv=None, max_steps=100, lr=0.001, scale=0.25, num_rays=None, target=None):
        """poses (B, 4, 4) fp32 / fp64 on the device, all against the frame `data` and the same pixels `uv` ((Rp, 2), x then y; drawn by `sample_pixels` when
        None) -> dict of device tensors: T_c2w (B, 4, 4) fp64, T_c2w32 fp32, loss_init, loss_last (B) fp64, accepted, nan (B) int32, grad (B, 6) fp64 (the
        last step's gradient of the loss with respect to the se(3) vector).  A pose whose loss became NaN, or ended above its first value, comes back as given.
        target: optionally the (Rp, C) values to compare with, instead of sampling data['feat_pyramid']['layer1'] / data['img'].
        The library loop makes no host synchronisation once the frame's tables exist and the shape has been captured (both happen on the first call)."""
        if not torch.is_tensor(poses) or not poses.is_cuda:
            raise RuntimeError("PoseOptimizer.refine: poses on a HIP device (the renderer has no CPU path)")
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or not 1 <= poses.shape[0] <= RL.MAX_POSES or poses.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"PoseOptimizer.refine: poses (B, 4, 4), fp32 or fp64, 1 <= B <= {RL.MAX_POSES}")
        net = self.nerf_renderer.eval()
        dev = poses.device
        K = data['K'].detach().to(dev, torch.float32).clone()
        H, W = data['img'].shape[-2:]
        if scale is not None:
            K[:2] *= scale
            H, W = int(H * scale), int(W * scale)
        if uv is None:
            uv = self.sample_pixels(data, H, W, num_rays)
        uv = uv.to(dev, torch.float32).contiguous()
        rargs = net.args.render
        white = bool(data.get("white_bkgd", rargs.white_bkgd))
        gk = lease = None
        if self.hip_loop and rargs.N_importance == 0 and diff_render.USE_GRAPHS and diff_render.KEEP_BYTES:
            with torch.no_grad():
                r = net._ensure_frame(data, "fine")
            if self._plan is not None and (self._plan.gk.r is not r or self._plan.gk.gen != r.state_gen):
                self._plan = None   # another frame or weight set: the old static workspace (gigabytes) goes before the new one is made
            gk = r.keep_buffers(poses.shape[0] * uv.shape[0], white, max_bytes=diff_render.KEEP_BYTES)
            lease = gk.acquire() if gk is not None else None   # None: a forward pass of this shape still waits for its backward — the buffers are not ours to use
        if lease is None:
            return self._refine_eager(poses, data, uv, K, H, W, max_steps, lr, target)
        try:
            return self._refine_hip(r, gk, poses.contiguous(), data, uv, K, H, W, max_steps, lr, target)
        finally:
            lease.release()   # (every later user of the buffers enqueues behind this refinement on the same stream)

    def _target_map(self, data):
        return data['feat_pyramid']['layer1'] if self.use_feat else data['img']

    def _refine_hip(self, r, gk, poses, data, uv, K, H, W, max_steps, lr, target):
        net, dev = self.nerf_renderer, poses.device
        B, Rp = int(poses.shape[0]), int(uv.shape[0])
        okey, gkey = ("feat", "g_feat") if self.use_feat else ("rgb", "g_rgb")
        C = int(gk.out[okey].shape[1])
        with torch.no_grad(), torch.cuda.device(dev):
            key = (id(gk), r.state_gen, r.precision, B, Rp, okey, float(lr))
            plan = self._plan
            if plan is None or plan.key != key:
                plan = self._plan = _Plan(key, gk, B, Rp, C, dev)
            plan.K.copy_(K)
            plan.uv.copy_(uv)
            tgt = RL.sample_target(self._target_map(data).detach(), H, W, plan.uv) if target is None else target.to(dev, torch.float32)
            if tuple(tgt.shape) != (Rp, C):
                raise ValueError(f"PoseOptimizer.refine: the target has shape {tuple(tgt.shape)}, the renderer's '{okey}' output has {C} channels at {Rp} pixels")
            plan.target.copy_(tgt)
            near, far = data['depth_range'][0]
            gk.z.copy_(net.sample_depths(r.S, near, far).to(torch.float32).expand(B * Rp, r.S))
            for t in gk.cot.values():
                t.zero_()
            RL.init(poses, plan.state)

            def one_step():
                RL.pose_rays(plan.state, plan.K, plan.uv, Rp, plan.pose32, gk.o, gk.d, gk.q)
                gk.forward_inplace()
                RL.loss(gk.out[okey], gk.out["mask"], plan.target, B, Rp, gk.cot[gkey], plan.row_loss)
                gk.backward_inplace()
                RL.step(plan.state, plan.row_loss, gk.go, gk.gd, gk.gq, plan.K, plan.uv, Rp, C, lr, BETAS[0], BETAS[1], ADAM_EPS)

            todo = int(max_steps)
            if not self.capture:
                for _ in range(todo):
                    one_step()
            else:
                if plan.graph is None and todo >= 1:
                    one_step()   # the warm step: the frame's tables that are built on first use exist before the capture
                    todo -= 1
                    if todo >= 1:
                        self._capture(plan, one_step)
                if plan.graph is not None:
                    for _ in range(todo):
                        plan.graph.replay()
            T64, T32, info = RL.finish(plan.state)
            out = {"T_c2w": T64, "T_c2w32": T32, "loss_init": info[:, 0].clone(), "loss_last": info[:, 1].clone(), "accepted": info[:, 2].to(torch.int32),
                   "nan": info[:, 3].to(torch.int32), "grad": plan.state[:, RL.S_GRAD].clone(), "path": "hip"}
        return out

    @staticmethod
    def _capture(plan, one_step):
        """One step as a HIP graph, captured on the plan's side stream (the libraries only enqueue on the stream they are given; nothing allocates in a step)."""
        cur = torch.cuda.current_stream(plan.stream.device)
        plan.stream.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(plan.stream):
            g.capture_begin()
            try:
                one_step()
            finally:
                g.capture_end()
        cur.wait_stream(plan.stream)
        plan.graph = g

    # ------------------------------------------------------------------ the eager formulation (pose_optimizer.py:75-199)
    def _refine_eager(self, poses, data, uv, K, H, W, max_steps, lr, target):
        net, dev = self.nerf_renderer, poses.device
        uvl = uv.long()
        if target is not None:
            tgt = target.to(dev, torch.float32)
        else:
            m = self._target_map(data).detach()
            m = m if m.dim() == 4 else m[None]
            if tuple(m.shape[-2:]) != (H, W) or self.use_feat:
                m = F.interpolate(m, size=(H, W), mode='bilinear', align_corners=False)
            tgt = m.permute(0, 2, 3, 1)[0][uvl[:, 1], uvl[:, 0]]
        okey = "feat" if self.use_feat else "rgb"
        res = {k: [] for k in ("T_c2w", "loss_init", "loss_last", "accepted", "nan", "grad")}
        for pose in poses:
            params = se3_log_map(pose.float()[None]).detach().requires_grad_(True)
            opt = torch.optim.Adam(params=[params], lr=lr, betas=BETAS)
            zero = torch.zeros((), device=dev)
            loss_init, loss, nan = None, zero, False
            with torch.enable_grad():
                for _ in range(int(max_steps)):
                    cam_pose = se3_exp_map(params)[0]
                    rays = net.points_2d_to_rays(uv, H, W, K, cam_pose)
                    rays['depth_range'] = data['depth_range'][0]
                    d2 = dict(data)
                    d2.update({'pose': cam_pose, 'K': K})
                    output = net.render_rays(d2, rays)
                    loss = torch.mean(((output[okey] - tgt) * output['mask'].unsqueeze(1)) ** 2)
                    if bool(loss.isnan().any()):
                        nan = True
                        break
                    if loss_init is None:
                        loss_init = loss.detach()
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
            loss = loss.detach()
            loss_init = loss if loss_init is None else loss_init
            accepted = not nan and not bool(loss > loss_init)
            T = se3_exp_map(params.detach().double())[0] if accepted else pose.double()
            grad = torch.zeros(6, device=dev, dtype=torch.float64) if params.grad is None else params.grad[0].double()
            for k, v in (("T_c2w", T), ("loss_init", loss_init.double()), ("loss_last", loss.double()), ("accepted", torch.tensor(int(accepted), dtype=torch.int32, device=dev)),
                         ("nan", torch.tensor(int(nan), dtype=torch.int32, device=dev)), ("grad", grad)):
                res[k].append(v)
        out = {k: torch.stack(v) for k, v in res.items()}
        out["T_c2w32"] = torch.stack([T.float() if a else p.float() for T, a, p in zip(out["T_c2w"], out["accepted"].tolist(), poses)])
        out["path"] = "eager"
        return out
