"""GPU tests of the pose refinement: libnerfloc_refine.so's kernels against the fp64 restatement tests/refine_ref.py at the shapes where they can go wrong (one ray,
one wave's worth, a non-multiple of the wave; 1 and 3 poses; scalar and 16-byte channel paths), nlr_sample_target against torch's own bilinear resize in fp64,
and nerf_loc_amd.pose_optimizer.PoseOptimizer on the `setup` scene of tests/golden_cases.py (24 rays, 16 samples, W 32, 3 views, 32 x 48 image) in "fp32".
fp32 outputs are held to 1e-6 of max |ref| (only the store rounds), fp64 outputs to 1e-10 (the summation order and the device's sin / cos differ), integers and
latches exactly."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_loc_amd import _refine_lib as RL
from nerf_loc_amd import pose_optimizer as po
from tests import refine_ref as rr

pytestmark = pytest.mark.gpu
BAR = 1e-4   # the project's parity bar
F32_TOL, F64_TOL = 1e-6, 1e-10
SHIFT = (0.01, -0.015, 0.02)
K_TEST = np.array([[40.0, 0, 23.5], [0, 42.0, 15.5], [0, 0, 1]], np.float32)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a, b = a.astype(np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def poses_of(B, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((B, 6)) * np.array([1.0, 1.0, 1.0, 0.4, 0.4, 0.4])
    return p, np.stack([rr.se3_exp(q) for q in p])


def pixels(Rp, seed):
    """Fractional and border coordinates of a 48 x 32 image."""
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(0, 47.99, Rp), rng.uniform(0, 31.99, Rp)], 1).astype(np.float32)
    for i, v in enumerate([(0, 0), (47.99, 31.99), (47, 0), (0.5, 31)][:Rp]):
        uv[i] = v
    return uv


# ------------------------------------------------------------------------------------------ the kernels alone
def test_se3_kernels_against_the_restatement_on_the_golden_cases():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_se3.npz"))
    names = [str(n) for n in g["names"]]
    p = np.stack([g[f"{n}.p"] for n in names])
    Gc = np.stack([g[f"{n}.G"] for n in names])
    T = RL.se3_exp(dev(p))
    gp = RL.se3_exp_backward(dev(p), dev(Gc))
    lg = RL.se3_log(dev(np.stack([g[f"{n}.T"] for n in names] + [g["identity.T"]])))
    for i, n in enumerate(names):
        assert err(T[i], g[f"{n}.T"]) <= F64_TOL and err(T[i], rr.se3_exp(p[i])) <= F64_TOL, n
        assert err(gp[i], g[f"{n}.grad"]) <= F64_TOL and err(gp[i], rr.se3_exp_backward(p[i], Gc[i])) <= F64_TOL, n
        assert err(lg[i], g[f"{n}.log"]) <= F64_TOL, n
    assert float(lg[-1].abs().max()) == 0.0
    assert bits(RL.se3_exp(dev(p))) == bits(T) and RL.se3_exp(dev(np.zeros((0, 6)))).shape == (0, 4, 4)


@pytest.mark.parametrize("pose_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,Rp", [(1, 1), (1, 24), (1, 77), (3, 1), (3, 24), (3, 77)])
def test_init_rays_step_finish_against_the_restatement(B, Rp, pose_dtype):
    C = 5
    _, T = poses_of(B, 10 + B)
    given = dev(T, pose_dtype)
    T_in = given.cpu().numpy().astype(np.float64)
    uv, K = pixels(Rp, Rp), K_TEST
    state = RL.new_state(B, "cuda")
    state.fill_(float("nan"))
    RL.init(given, state)
    ref = [rr.init_state(t) for t in T_in]
    s = state.cpu().numpy()
    for b in range(B):
        assert err(s[b, RL.S_PARAMS], ref[b]["params"]) <= F64_TOL
        assert np.array_equal(s[b, RL.S_POSE0].reshape(4, 4), T_in[b]) and not s[b, 6:26].any()
    assert not state.view(torch.int64)[:, [RL.S_T, RL.S_NAN]].any()
    # rays
    R = B * Rp
    o, d, c, p32 = [torch.full((R, 3), float("nan"), device="cuda") for _ in range(3)] + [torch.empty(B, 4, 4, device="cuda")]
    RL.pose_rays(state, dev(K), dev(uv), Rp, p32, o, d, c)
    for b in range(B):
        ro, rd, rc = rr.pose_rays(rr.se3_exp(ref[b]["params"]), K, uv)
        sl = slice(b * Rp, (b + 1) * Rp)
        assert err(o[sl], ro) <= F32_TOL and err(d[sl], rd) <= F32_TOL and bits(o[sl]) == bits(c[sl])
        assert err(p32[b], rr.se3_exp(ref[b]["params"])) <= F32_TOL
    # two steps; in the second one the last pose of three meets a NaN loss and latches; a third step leaves it alone
    rng = np.random.default_rng(Rp)
    for it in range(3):
        row_loss = rng.random(R) + 0.5
        if it == 1 and B == 3:
            row_loss[2 * Rp + Rp // 2] = np.nan
        g_o, g_d, g_c = (rng.standard_normal((3, R, 3)) * 0.1).astype(np.float32)
        RL.step(state, dev(row_loss), dev(g_o), dev(g_d), dev(g_c), dev(K), dev(uv), Rp, C, lr=2e-3)
        s = state.cpu().numpy()
        si = state.view(torch.int64).cpu().numpy()
        for b in range(B):
            sl = slice(b * Rp, (b + 1) * Rp)
            rr.step(ref[b], row_loss[sl], C, g_o[sl], g_d[sl], g_c[sl], K, uv, lr=2e-3)
            for name, cols in (("params", RL.S_PARAMS), ("m", RL.S_M), ("v", RL.S_V), ("grad", RL.S_GRAD)):
                assert err(s[b, cols], ref[b][name]) <= F64_TOL, (it, b, name)
            assert si[b, RL.S_T] == ref[b]["t"] and si[b, RL.S_NAN] == ref[b]["nan"]
            assert err(s[b, RL.S_LOSS_INIT], ref[b]["loss_init"]) <= F64_TOL
            assert (np.isnan(s[b, RL.S_LOSS_LAST]) and np.isnan(ref[b]["loss_last"])) or err(s[b, RL.S_LOSS_LAST], ref[b]["loss_last"]) <= F64_TOL
    assert [r["nan"] for r in ref] == ([0, 0, 1] if B == 3 else [0]) and [r["t"] for r in ref] == ([3, 3, 1] if B == 3 else [3])
    T64, T32, info = RL.finish(state)
    for b in range(B):
        want, accepted = rr.finish(ref[b])
        assert int(info[b, 2]) == accepted and int(info[b, 3]) == ref[b]["nan"]
        if accepted:
            assert err(T64[b], want) <= F64_TOL and err(T32[b], want) <= F32_TOL
        else:   # the pose as given, bit for bit
            assert np.array_equal(T64[b].cpu().numpy(), T_in[b]) and bits(T32[b]) == T_in[b].astype(np.float32).tobytes()
            if pose_dtype == torch.float32:
                assert bits(T32[b]) == bits(given[b])


@pytest.mark.parametrize("C", [3, 5, 192])
@pytest.mark.parametrize("B,Rp", [(1, 1), (1, 24), (1, 77), (3, 1), (3, 24), (3, 77)])
def test_loss_against_the_restatement(B, Rp, C):
    rng = np.random.default_rng(B * 1000 + Rp * 10 + C)
    R = B * Rp
    out, tgt = rng.standard_normal((R, C)).astype(np.float32), rng.standard_normal((Rp, C)).astype(np.float32)
    mask = (rng.random(R) > 0.3).astype(np.uint8)
    mask[0] = 1
    if B > 1:
        mask[(B - 1) * Rp:] = 0   # all false for one pose of several; a single pose meets the all-false mask in a call of its own below
    g = torch.full((R, C), float("nan"), device="cuda")
    rows = torch.full((R,), float("nan"), device="cuda", dtype=torch.float64)
    RL.loss(dev(out), dev(mask), dev(tgt), B, Rp, g, rows)
    for b in range(B):
        sl = slice(b * Rp, (b + 1) * Rp)
        wr, wg = rr.loss_rows(out[sl], mask[sl], tgt)
        assert err(rows[sl], wr) <= F64_TOL if wr.any() else not rows[sl].any()
        assert err(g[sl], wg) <= F32_TOL if wg.any() else not g[sl].any()
    assert float(rows[0]) > 0 and bool(g[0].any())
    g2, rows2 = torch.full_like(g, float("nan")), torch.full_like(rows, float("nan"))
    RL.loss(dev(out), dev(np.zeros(R, np.uint8)), dev(tgt), B, Rp, g2, rows2)
    assert not g2.any() and not rows2.any()   # every pose masked out: zeros, not NaN
    RL.loss(dev(out), dev(mask).view(torch.bool), dev(tgt), B, Rp, g2, rows2)
    assert bits(g2) == bits(g) and bits(rows2) == bits(rows)
    if C % 4 == 0:   # a row start that is not 16-byte aligned takes the scalar path: the same values
        pad = torch.zeros(R * C + 1, device="cuda")
        pad[1:] = dev(out).reshape(-1)
        RL.loss(pad[1:].view(R, C), dev(mask), dev(tgt), B, Rp, g2, rows2)
        assert err(rows2, rows.cpu().numpy()) <= F64_TOL and bits(g2) == bits(g)


@pytest.mark.parametrize("C", [3, 192])
@pytest.mark.parametrize("src,dst", [((5, 7), (32, 48)), ((32, 48), (8, 12))])
def test_sample_target_against_interpolate(src, dst, C):
    rng = np.random.default_rng(C + src[0])
    (h, w), (H, W) = src, dst
    m = rng.standard_normal((1, C, h, w)).astype(np.float32)
    full = F.interpolate(torch.from_numpy(m).double(), size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    uv = np.stack([rng.uniform(0, W - 0.01, 40), rng.uniform(0, H - 0.01, 40)], 1).astype(np.float32)
    uv[:4] = [[0, 0], [W - 1, 0], [0, H - 1], [W - 0.5, H - 0.5]]
    want = full[:, uv[:, 1].astype(int), uv[:, 0].astype(int)].T
    nchw = dev(m)
    nhwc = nchw.contiguous(memory_format=torch.channels_last)
    a, b = RL.sample_target(nchw, H, W, dev(uv)), RL.sample_target(nhwc, H, W, dev(uv))
    assert a.shape == (40, C) and err(a, want) <= F32_TOL and err(a, rr.sample_target(m[0], H, W, uv)) <= F32_TOL
    assert bits(a) == bits(b) and bits(RL.sample_target(nchw[0], H, W, dev(uv))) == bits(a)
    if C > 1:
        assert nhwc.stride() != nchw.stride()


# ------------------------------------------------------------------------------------------ the loop on the `setup` scene
def _args(cfg):
    return NS(multires=10, multires_views=4, i_embed=0, backbone2d_fpn_dim=cfg.C, model_3d_hidden_dim=cfg.W,
              render=NS(N_samples=cfg.S, N_importance=cfg.N_importance, N_rand=1024, chunk=2048, lindisp=bool(cfg.lindisp), white_bkgd=False,
                        use_render_uncertainty=True, render_feature=True),
              use_scene_coord_memorization=False, matcher_hidden_dim=192, use_depth_supervision=False, matching=NS(fine_num_3d_keypoints=1024))


def _module(case, cfg):
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    net = ConditionalNeRF(_args(cfg), precision="fp32").to("cuda:0").eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case["weights"].items()}, strict=True)
    return net


@functools.lru_cache(maxsize=None)
def scene():
    """The module, the frame, the golden pixels and the render at the true pose, made once."""
    from tests.golden_cases import build_setup_case
    case = build_setup_case("setup")
    cfg, frame = case["cfg"], case["frame"]
    net = _module(case, cfg)
    data = {k: dev(frame[k]) for k in ("topk_images", "topk_depths", "topk_Ks", "topk_poses", "feat_fine_src", "feat_coarse_src", "depth_range", "K", "pose")}
    data.update({"embedding_a": None, "H": frame["H"], "W": frame["W"], "stride_fine": 4, "stride_coarse": 8})
    rng = np.random.default_rng(4)
    data["img"] = dev(rng.random((3, cfg.H, cfg.Wimg)).astype(np.float32))
    data["feat_pyramid"] = {"layer1": dev(rng.standard_normal((1, cfg.C, cfg.H // 4, cfg.Wimg // 4)).astype(np.float32))}
    rays = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case["rays"].items()}
    with torch.no_grad():
        true = net.render_rays(data, rays)
    assert int(true["mask"].sum()) == 22
    return NS(case=case, cfg=cfg, net=net, data=data, uv=rays["pixel_coordinates"], true=true, pose=data["pose"].clone())


def shifted(pose, shift=SHIFT, scale=1.0):
    p = pose.clone()
    p[:3, 3] += torch.tensor(shift, device=p.device, dtype=p.dtype) * scale
    return p


def masked_in(s, pose, uv=None, net=None):
    """How many of the rays through `uv` (default: the golden pixels) the renderer's mask keeps at `pose`: every loop test wants at least half of its rays at
    its start pose."""
    uv, net = s.uv if uv is None else uv, net or s.net
    with torch.no_grad():
        rays = net.points_2d_to_rays(uv, s.cfg.H, s.cfg.Wimg, s.data["K"], pose)
        rays["depth_range"] = s.data["depth_range"][0]
        return int(net.render_rays({**s.data, "pose": pose}, rays)["mask"].sum())


def optimizer(s, **kw):
    return po.PoseOptimizer(s.net.args, s.net, **kw)


def run(s, opt, poses, steps, target="feat", **kw):
    tgt = s.true[target] if isinstance(target, str) else target
    return opt.refine(poses, s.data, uv=s.uv, max_steps=steps, lr=2e-3, scale=None, target=tgt, **kw)


def test_one_step_gradient_against_autograd_of_the_eager_formulation():
    s = scene()
    start = shifted(s.pose)
    assert masked_in(s, start) >= 12
    opt = optimizer(s)
    hip = run(s, opt, start[None], 1)
    opt.hip_loop = False
    eager = run(s, opt, start[None], 1)
    assert hip["path"] == "hip" and eager["path"] == "eager"
    g, ge = hip["grad"][0].cpu().numpy(), eager["grad"][0].cpu().numpy()
    e = np.abs(g - ge).max() / np.abs(ge).max()
    print(f"one-step pose gradient, library loop vs eager autograd: max |dg| / max |g| = {e:.3e}; loss {float(hip['loss_init'][0]):.6e} vs {float(eager['loss_init'][0]):.6e}")
    assert np.abs(ge).max() > 0 and e <= BAR
    assert err(hip["loss_init"], eager["loss_init"].cpu().numpy()) <= BAR and int(hip["nan"][0]) == 0


def test_twelve_steps_reduce_the_loss_and_approach_the_true_pose():
    s = scene()
    start = shifted(s.pose)
    assert masked_in(s, start) >= 12
    out = run(s, optimizer(s), start[None].double(), 12)
    li, ll = float(out["loss_init"][0]), float(out["loss_last"][0])
    print(f"12 steps: loss {li:.6e} -> {ll:.6e}")
    assert ll < 0.7 * li and int(out["accepted"][0]) == 1 and int(out["nan"][0]) == 0
    t_true = s.pose[:3, 3].double()
    assert float((out["T_c2w"][0, :3, 3] - t_true).norm()) < float((start[:3, 3].double() - t_true).norm())
    assert out["T_c2w"].dtype == torch.float64 and out["T_c2w32"].dtype == torch.float32 and err(out["T_c2w32"], out["T_c2w"].cpu().numpy()) <= F32_TOL


def test_bit_for_bit_repeat_uncaptured_and_batched():
    s = scene()
    starts = torch.stack([shifted(s.pose), shifted(s.pose, scale=0.5), shifted(s.pose, (-0.01, 0.005, 0.01))])
    for p in starts:
        assert masked_in(s, p) >= 12
    opt = optimizer(s)
    keys = ("T_c2w", "T_c2w32", "loss_init", "loss_last", "accepted", "nan", "grad")
    a = run(s, opt, starts[:1], 5)
    b = run(s, opt, starts[:1], 5)
    assert opt._plan.graph is not None
    plain = optimizer(s)
    plain.capture = False
    c = run(s, plain, starts[:1], 5)
    assert plain._plan.graph is None
    for k in keys:
        assert bits(a[k]) == bits(b[k]) == bits(c[k]), k
    three = run(s, optimizer(s), starts, 5)
    singles = [run(s, opt, starts[i:i + 1], 5) for i in range(3)]
    for k in keys:
        assert bits(three[k]) == b"".join(bits(x[k]) for x in singles), k
    assert len({bits(three["T_c2w"][i]) for i in range(3)}) == 3


def test_no_steps_give_exp_of_log():
    s = scene()
    start = shifted(s.pose)
    out = run(s, optimizer(s), start[None], 0)
    want = rr.se3_exp(rr.se3_log(start.cpu().numpy().astype(np.float64)))
    same64 = np.array_equal(out["T_c2w"][0].cpu().numpy(), want)
    print(f"max_steps=0: fp64 bits equal to the numpy restatement: {same64}; max deviation {err(out['T_c2w'][0], want):.3e}")
    # bit for bit, fp64 and fp32: the restatement writes every sum and the adjugate in the header's order
    assert same64 and bits(out["T_c2w32"][0]) == want.astype(np.float32).tobytes()
    assert int(out["accepted"][0]) == 1 and float(out["loss_init"][0]) == 0.0 == float(out["loss_last"][0])


def test_discard_rules():
    s = scene()
    start = shifted(s.pose)
    opt = optimizer(s)
    bad = s.true["feat"].clone()
    inside = int(torch.nonzero(s.true["mask"])[0])
    bad[inside, 1] = float("nan")
    assert masked_in(s, start) >= 12
    for given in (start[None], start[None].double()):
        out = run(s, opt, given, 4, target=bad)
        assert int(out["nan"][0]) == 1 and int(out["accepted"][0]) == 0
        assert bits(out["T_c2w"][0]) == bits(given[0].double()) and bits(out["T_c2w32"][0]) == bits(given[0].float())
    # from the true pose against its own render the loss can only rise
    assert masked_in(s, s.pose) >= 12
    out = run(s, opt, s.pose[None], 4)
    print(f"from the true pose: loss {float(out['loss_init'][0]):.3e} -> {float(out['loss_last'][0]):.3e}")
    assert int(out["accepted"][0]) == 0 and int(out["nan"][0]) == 0 and float(out["loss_last"][0]) > float(out["loss_init"][0])
    assert bits(out["T_c2w32"][0]) == bits(s.pose) and bits(out["T_c2w"][0]) == bits(s.pose.double())


@pytest.mark.parametrize("use_feat", [True, False])
def test_call_with_grid_sampling_equals_refine_on_the_same_pixels(use_feat):
    s = scene()
    start = shifted(s.pose)
    opt = optimizer(s, sampling="grid", use_feat=use_feat)
    got = opt(start.cpu().numpy()[:3], s.data, max_steps=3, lr=2e-3, scale=None)
    ys, xs = np.meshgrid(np.arange(0, s.cfg.H, 10), np.arange(0, s.cfg.Wimg, 10), indexing="ij")
    uv = dev(np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32))
    inside = masked_in(s, start, uv)
    print(f"grid pixels masked in at the start pose: {inside} of {len(uv)}")
    assert len(uv) == 20 and 2 * inside >= len(uv)
    want = opt.refine(start[None], s.data, uv=uv, max_steps=3, lr=2e-3, scale=None)
    assert got.shape == (4, 4) and got.dtype == torch.float32 and got.is_cuda and bits(got) == bits(want["T_c2w32"][0])
    assert want["path"] == "hip" and float(want["loss_init"][0]) > 0
    # ... and the target it compared with is the frame's own map at those pixels
    m = s.data["feat_pyramid"]["layer1"] if use_feat else s.data["img"][None]
    full = F.interpolate(m.double().cpu(), size=(s.cfg.H, s.cfg.Wimg), mode="bilinear", align_corners=False)[0].numpy()
    assert err(opt._plan.target, full[:, ys.reshape(-1), xs.reshape(-1)].T) <= F32_TOL
    np.random.seed(3)
    rnd = optimizer(s, sampling="random", num_rays=16)
    a = rnd.sample_pixels(s.data, s.cfg.H, s.cfg.Wimg)
    np.random.seed(3)
    idx = np.random.choice(s.cfg.H * s.cfg.Wimg, 16, replace=False)
    assert a.shape == (16, 2) and np.array_equal(a.numpy(), np.stack([idx // s.cfg.H, idx % s.cfg.H], 1))


def test_eager_formulation_runs_where_the_library_loop_does_not(monkeypatch):
    s = scene()
    start = shifted(s.pose)
    for fn in ("init", "pose_rays", "sample_target", "loss", "step", "finish", "new_state"):
        monkeypatch.setattr(RL, fn, lambda *a, **k: pytest.fail("the library loop was entered"))
    opt = optimizer(s)
    opt.hip_loop = False
    assert masked_in(s, start) >= 12
    out = opt.refine(start[None], s.data, uv=s.uv, max_steps=2, lr=2e-3, scale=None)
    assert out["path"] == "eager" and out["T_c2w"].shape == (1, 4, 4) and out["T_c2w32"].dtype == torch.float32 and int(out["nan"][0]) == 0
    assert set(out) == {"T_c2w", "T_c2w32", "loss_init", "loss_last", "accepted", "nan", "grad", "path"}
    # keep buffers held by a forward pass that still waits for its backward: eager for that call, the library loop again once they are free
    busy = optimizer(s)
    gk = s.net._ensure_frame(s.data, "fine").keep_buffers(len(s.uv), False)
    lease = gk.acquire()
    assert lease is not None and gk.acquire() is None
    assert busy.refine(start[None], s.data, uv=s.uv, max_steps=1, lr=2e-3, scale=None, target=s.true["feat"])["path"] == "eager"
    lease.release()
    lease = gk.acquire()   # and refine gave nothing away that was not its own
    assert lease is not None
    del lease
    # a module that resamples hierarchically redraws its samples every step: eager, whatever hip_loop says
    from nerf_loc_amd.synth import make_depth_fusion_weights, make_weights
    cfg = s.cfg.replace(N_importance=16)   # (the ray U-Net's LayerNorm tables follow the sample count: weights of their own)
    net = _module({"weights": {**make_weights(cfg), **make_depth_fusion_weights(cfg.seed)}}, cfg)
    hier = po.PoseOptimizer(net.args, net)
    assert hier.hip_loop and masked_in(s, start, net=net) >= 12
    out = hier.refine(start[None], s.data, uv=s.uv, max_steps=1, lr=2e-3, scale=None, target=s.true["feat"])
    assert out["path"] == "eager" and bool(torch.isfinite(out["T_c2w"]).all())


def test_refine_does_not_synchronise(monkeypatch):
    s = scene()
    start = shifted(s.pose)
    opt = optimizer(s)
    assert masked_in(s, start) >= 12
    first = opt.refine(start[None].double(), s.data, uv=s.uv, max_steps=3, lr=2e-3, scale=None)   # builds the frame's tables, captures the shape

    def forbidden(*a, **k):
        raise AssertionError("a host synchronisation inside refine")
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        mp.setattr(torch.Tensor, "item", forbidden)
        mp.setattr(torch.Tensor, "cpu", forbidden)
        again = opt.refine(start[None].double(), s.data, uv=s.uv, max_steps=3, lr=2e-3, scale=None)
    assert again["path"] == "hip" and bits(again["T_c2w"]) == bits(first["T_c2w"]) and all(v.is_cuda for k, v in again.items() if k != "path")
