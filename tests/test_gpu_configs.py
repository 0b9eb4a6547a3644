"""Every BASELINE.json configuration on the GPU against the CPU oracle (run with `pytest -m gpu`).

c2 has its own full-size tests in test_gpu_parity.py.  Here: c3 (8192 x 128), c4 (16384 x 192, 256x448 views, outdoor depth range
0.25 / 25) and c5 (hierarchical 64 coarse + 64 + 128 resampled, 16 views): a sample of the rays of the full-size workload against
`oracle.render_rays` at BASELINE's 1e-4 (max-rel-to-max AND L2-relative), plus size-independent properties of the WHOLE batch
(finite, weights sum to 1, depth inside the range, determinism, invariance of a ray's result to the batch it is rendered in)."""
import numpy as np
import pytest
import torch

from tests.util import l2_rel, rel_err, surface_weights

pytestmark = pytest.mark.gpu
KEYS = ("rgb", "depth", "weights", "depth_uncertainty", "feat")


def _scene(name):
    from nerf_loc_amd.synth import CONFIGS, make_frame, make_rays, make_u, make_weights
    cfg = CONFIGS[name]
    frame = make_frame(cfg)
    return {"cfg": cfg, "frame": frame, "rays": make_rays(cfg, frame), "weights": make_weights(cfg), "u": make_u(cfg)}


def _renderer(sc, precision):
    from nerf_loc_amd.renderer import HipRenderer
    cfg, fr = sc["cfg"], sc["frame"]
    r = HipRenderer(cfg.W, cfg.C, cfg.S_total, precision)
    r.load_weights({k: torch.from_numpy(v) for k, v in sc["weights"].items()})
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])
    return r


def _zbase(cfg, R):
    from oracle.render_oracle import sample_depths
    return sample_depths(cfg.S, torch.tensor(cfg.near), torch.tensor(cfg.far)).expand(R, cfg.S).contiguous()


def _render(r, sc, sel=None, precision_note=""):
    cfg = sc["cfg"]
    o, d = sc["rays"]["rays_o"], sc["rays"]["rays_d"]
    pix, u = sc["rays"]["pixel_coordinates"], sc["u"]
    if sel is not None:
        o, d, pix, u = o[sel], d[sel], pix[sel], u[sel]
    z = _zbase(cfg, len(o))
    extra = {}
    if cfg.N_importance > 0:
        z, dc, _ = r.hierarchical_depths(pix, sc["frame"]["K"], sc["frame"]["pose"], z, u, near=cfg.near, far=cfg.far)
        extra["depth_coarse"] = dc
    out = r.render_rays(o, d, sc["frame"]["pose"][:3, 3], z_vals=z, white_bkgd=cfg.white_bkgd)
    out.update(extra)
    return out


def _oracle(sc, sel, threads=16):
    from oracle import render_oracle as orc
    cfg = sc["cfg"]
    params = {k: torch.from_numpy(v) for k, v in sc["weights"].items()}
    sub = {k: (torch.from_numpy(v[sel]) if k in ("rays_o", "rays_d", "pixel_coordinates") else (torch.from_numpy(v) if isinstance(v, np.ndarray) else v))
           for k, v in sc["rays"].items()}
    torch.set_num_threads(threads)
    with torch.no_grad():
        return orc.render_rays(params, orc.to_torch(sc["frame"]), sub, cfg.S, cfg.N_importance, u=torch.from_numpy(sc["u"][sel]), knn_threads=threads)


@pytest.fixture(scope="module", params=["c3", "c4", "c5"])
def scene(request):
    return _scene(request.param)


def test_sampled_rays_of_the_full_workload_match_oracle(scene):
    cfg = scene["cfg"]
    n = 48 if cfg.S_total > 128 else 64
    sel = np.arange(0, cfg.R, cfg.R // n)[:n]
    ref = _oracle(scene, sel)
    r = _renderer(scene, "bf16x3")
    keys = KEYS + (("depth_coarse",) if cfg.N_importance > 0 else ())
    for prec in ("f16mx", "bf16x3"):   # both parity modes (f16mx: the headline mode since round 4)
        r.set_precision(prec)
        out = _render(r, scene, sel)
        assert np.array_equal(out["mask"].cpu().numpy(), ref["mask"].numpy())
        errs = {k: (rel_err(out[k].cpu().numpy(), ref[k].numpy()), l2_rel(out[k].cpu().numpy(), ref[k].numpy())) for k in keys}
        assert all(e[0] < 1e-4 and e[1] < 1e-4 for e in errs.values()), (cfg.name, prec, errs)
    # throughput mode (single bf16 MFMA per product): does NOT meet 1e-4 — its error is measured and bounded, not hidden
    r.set_precision("bf16")
    fast = _render(r, scene, sel)
    e16 = {k: rel_err(fast[k].cpu().numpy(), ref[k].numpy()) for k in KEYS}
    print(f"\n{cfg.name} bf16x3 (max-rel, l2-rel): {errs}\n{cfg.name} bf16 max-rel: {e16}")
    assert max(e16.values()) < 3e-2, (cfg.name, e16)


@pytest.mark.parametrize("prec", ["f16mx", "bf16x3"])
def test_full_size_batch_properties(scene, prec):
    cfg = scene["cfg"]
    r = _renderer(scene, prec)
    a = _render(r, scene)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.isfinite(a[k]).all(), k
    assert a["rgb"].shape == (cfg.R, 3) and a["weights"].shape == (cfg.R, cfg.S_total)
    assert float((a["weights"].sum(1) - 1).abs().max()) < 1e-4          # last delta = 1e2 makes every ray opaque (model.py:544-553)
    assert float(a["depth"].min()) >= cfg.near - 1e-3 and float(a["depth"].max()) <= cfg.far + 1e-3
    b = _render(r, scene)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), ("determinism", k)
    # a ray's result does not depend on the batch it is rendered in (what ray-range sharding over GPUs relies on)
    sel = np.arange(cfg.R // 2 - 100, cfg.R // 2 + 100)
    c = _render(r, scene, sel)
    for k in KEYS:
        assert torch.equal(a[k][torch.from_numpy(sel).to(a[k].device)], c[k]), ("shard invariance", k)


@pytest.mark.parametrize("name", ["c2", "c5"])
def test_early_termination_keeps_parity_and_skips_work(name):
    """BASELINE config 5 names early-termination compositing.  With eps = 1e-5 the colours / features of the samples behind the point
    where a ray's transmittance falls below eps are not evaluated: weights, depth, depth_uncertainty and mask are bit-identical,
    rgb / feat move by less than eps * max|value| (far inside 1e-4), and a real share of the samples is skipped."""
    sc = _scene(name)
    cfg = sc["cfg"]
    # random-init weights give a thin medium (alpha ~ 0.03 per sample: no ray ever gets opaque before its last sample), so the
    # density head's bias is raised to make surfaces (rung A of nerf_loc_amd.synth.SURFACE_RUNGS): sigma ~ 8 -> transmittance below 1e-5 after a few dozen samples
    sc["weights"], gain, offset = surface_weights(sc, "A")
    assert (gain, offset) == (1.0, 8.0)
    r = _renderer(sc, "bf16x3")
    sel = np.arange(0, cfg.R, 4)
    o, d = sc["rays"]["rays_o"][sel], sc["rays"]["rays_d"][sel]
    z = _zbase(cfg, len(sel))
    if cfg.N_importance > 0:
        z, _, _ = r.hierarchical_depths(sc["rays"]["pixel_coordinates"][sel], sc["frame"]["K"], sc["frame"]["pose"], z, sc["u"][sel], near=cfg.near, far=cfg.far)
    qc = sc["frame"]["pose"][:3, 3]
    full = r.render_rays(o, d, qc, z_vals=z)
    eps = 1e-5
    et = r.render_rays(o, d, qc, z_vals=z, early_term_eps=eps)
    for k in ("weights", "depth", "depth_uncertainty", "mask"):
        assert torch.equal(full[k], et[k]), k
    e_rgb = float((full["rgb"] - et["rgb"]).abs().max())
    e_feat = float((full["feat"] - et["feat"]).abs().max()) / float(full["feat"].abs().max())
    assert e_rgb < 1e-5 and e_feat < 2e-5, (e_rgb, e_feat)
    # share of samples whose transmittance is already below eps (what the option skips)
    w = full["weights"]
    T = 1.0 - torch.cumsum(w, 1) + w            # transmittance before each sample (sum of the later weights incl. itself, weights sum to 1)
    skipped = float((T < eps).float().mean())
    print(f"\n{name}: early termination eps={eps}: {100 * skipped:.1f} % of the samples skipped, |d rgb| {e_rgb:.2e}, rel |d feat| {e_feat:.2e}")
    assert skipped > 0.02


def test_render_opts_are_validated_and_streams_do_not_interfere():
    """(1) nl_render_opts with unknown flag bits / non-zero reserved words / a bad eps is refused on an otherwise valid call.  (2) The side
    stream belongs to the frame: two renderers (two frames) driven concurrently from two caller streams give results bit-identical to the
    same renders done one after the other, and identical with the fork switched off (NL_RENDER_NO_SIDE_STREAM)."""
    import ctypes as ct
    from nerf_loc_amd import _lib as L
    from nerf_loc_amd.synth import CONFIGS
    sc = _scene("c2")
    cfg = sc["cfg"].replace(R=1024)
    sc = dict(sc, cfg=cfg)
    ra, rb_ = _renderer(sc, "bf16x3"), _renderer(sc, "bf16x3")
    dev = ra.device
    o = torch.from_numpy(sc["rays"]["rays_o"][:1024]).to(dev)
    d = torch.from_numpy(sc["rays"]["rays_d"][:1024]).to(dev)
    d2 = torch.from_numpy(sc["rays"]["rays_d"][1024:2048]).to(dev)
    qc = sc["frame"]["pose"][:3, 3]
    z = _zbase(cfg, 1024).to(dev)
    # (1) validation with a live frame and valid pointers
    ws = torch.empty(ra.lib.nl_render_rays_workspace_bytes(ct.byref(ra.cfg), ra.V, 16), dtype=torch.uint8, device=dev)
    outbuf = {k: torch.empty(16, n, device=dev) for k, n in (("rgb", 3), ("depth", 1), ("weights", cfg.S), ("depth_uncertainty", 1))}
    ro = L.NlRenderOut()
    for k, t in outbuf.items():
        setattr(ro, k, t.data_ptr())
    qch = torch.as_tensor(qc).float().contiguous()

    def call(opts):
        return ra.lib.nl_render_rays_ex(ct.byref(ra.cfg), ra.packed.data_ptr(), ra._frame, qch.data_ptr(), o.data_ptr(), d.data_ptr(), None, 16, 0,
                                        ct.byref(ro), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream, ct.byref(opts))
    assert call(L.NlRenderOpts()) == L.NL_OK
    for bad in (dict(flags=4), dict(flags=0x80000000), dict(early_term_eps=float("nan")), dict(early_term_eps=1.0), dict(early_term_eps=-0.5)):
        op = L.NlRenderOpts()
        for k, v in bad.items():
            setattr(op, k, v)
        assert call(op) == L.NL_ERR_BAD_ARG, bad
    op = L.NlRenderOpts()
    op.reserved[3] = 1
    assert call(op) == L.NL_ERR_BAD_ARG
    torch.cuda.synchronize()
    # (2) serial reference, then both renderers at once on two streams
    ref_a = ra.render_rays(o, d, qc, z_vals=z)
    ref_b = rb_.render_rays(o, d2, qc, z_vals=z)
    nofork = ra.render_rays(o, d, qc, z_vals=z, side_stream=False)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(ref_a[k], nofork[k]), k
    from nerf_loc_amd.renderer import render_rays_concurrent
    both = render_rays_concurrent([(ra, o, d, qc, {"z_vals": z}), (rb_, o, d2, qc, {"z_vals": z})])
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(both[0][k], ref_a[k]) and torch.equal(both[1][k], ref_b[k]), k
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(5):
        with torch.cuda.stream(s1):
            ca = ra.render_rays(o, d, qc, z_vals=z)
        with torch.cuda.stream(s2):
            cb = rb_.render_rays(o, d2, qc, z_vals=z)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(ca[k], ref_a[k]) and torch.equal(cb[k], ref_b[k]), k


def test_ill_conditioned_visibility_sample_stays_inside_the_bar():
    """Regression for the sample tools/precision_budget.py found (round 3): among the first 32 rays of config 2's ray recipe one ray has samples whose
    ten views are all almost invisible, where the visibility weights' normalisation turns 7e-6 of decoder error (split-bf16) into 2.3e-4 on `weights`.
    With the decoders in split-FP16 the whole sample is far inside 1e-4."""
    from nerf_loc_amd.synth import CONFIGS, make_frame, make_rays, make_u, make_weights
    cfg = CONFIGS["c2"].replace(R=32)
    frame = make_frame(CONFIGS["c2"])
    sc = {"cfg": cfg, "frame": frame, "rays": make_rays(CONFIGS["c2"], frame, R=32), "weights": make_weights(CONFIGS["c2"]), "u": make_u(cfg)}
    sel = np.arange(32)
    ref = _oracle(sc, sel)
    out = _render(_renderer(sc, "bf16x3"), sc, sel)
    errs = {k: rel_err(out[k].cpu().numpy(), ref[k].numpy()) for k in KEYS}
    print(errs)
    assert max(errs.values()) < 5e-5, errs


def test_full_size_backward_properties():
    """nl_render_rays_backward at BASELINE config 2's full size (4096 rays x 128 samples = 524 288 samples, eight workspace chunks): size-independent
    properties of a backward pass — linear in the cotangents, bit-reproducible, and a ray's gradient does not depend on the batch / chunk it is
    differentiated in (what sharding a refinement batch over GPUs relies on)."""
    sc = _scene("c2")
    cfg = sc["cfg"]
    r = _renderer(sc, "bf16x3")
    dev = torch.device("cuda:0")
    o, d = torch.from_numpy(sc["rays"]["rays_o"]).to(dev), torch.from_numpy(sc["rays"]["rays_d"]).to(dev)
    z = _zbase(cfg, cfg.R).to(dev)
    qc = sc["frame"]["pose"][:3, 3]
    g = torch.Generator().manual_seed(31)
    grgb, gfeat, gdep = torch.randn(cfg.R, 3, generator=g).to(dev), torch.randn(cfg.R, cfg.C, generator=g).to(dev), torch.randn(cfg.R, generator=g).to(dev)
    a = r.render_rays_backward(o, d, z, qc, g_rgb=grgb, g_feat=gfeat, g_depth=gdep, want_g_query_center=True)
    b = r.render_rays_backward(o, d, z, qc, g_rgb=grgb, g_feat=gfeat, g_depth=gdep, want_g_query_center=True)
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y), "determinism"
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0
    # linearity: g(2 c1) = 2 g(c1) exactly (powers of two), g(c1 + c2) = g(c1) + g(c2) to rounding
    two = r.render_rays_backward(o, d, z, qc, g_rgb=2 * grgb, g_feat=2 * gfeat, g_depth=2 * gdep)
    assert torch.equal(two[0], 2 * a[0]) and torch.equal(two[1], 2 * a[1])
    p1 = r.render_rays_backward(o, d, z, qc, g_rgb=grgb)
    p2 = r.render_rays_backward(o, d, z, qc, g_feat=gfeat, g_depth=gdep)
    for k in (0, 1):
        assert rel_err((p1[k] + p2[k]).cpu().numpy(), a[k].cpu().numpy()) < 2e-5, k
    # a sub-batch (other chunk boundaries) gives the same rows
    sel = torch.arange(cfg.R // 2 - 150, cfg.R // 2 + 150, device=dev)
    c = r.render_rays_backward(o[sel], d[sel], z[sel], qc, g_rgb=grgb[sel], g_feat=gfeat[sel], g_depth=gdep[sel])
    for k in (0, 1):
        assert torch.equal(c[k], a[k][sel]), ("batch invariance", k)


def test_render_rays_multi_is_bit_identical_to_separate_calls():
    """nl_render_rays_multi (round 4): four frames with four different support sets — one of them used by two jobs, one job with per-ray query
    centres, ragged ray counts — in ONE library call against one nl_render_rays_ex call per job: every output bit for bit, in both parity modes."""
    from nerf_loc_amd.renderer import HipRenderer, render_rays_multi
    from nerf_loc_amd.synth import CONFIGS, make_frame, make_rays, make_weights
    cfg = CONFIGS["c1"].replace(R=96)
    weights = {k: torch.from_numpy(v) for k, v in make_weights(cfg).items()}
    dev = torch.device("cuda:0")
    for prec in ("bf16x3", "f16mx"):
        jobs = []
        for i in range(4):
            c = cfg.replace(seed=cfg.seed + 10 * i)
            fr = make_frame(c)
            r = HipRenderer(c.W, c.C, c.S_total, prec)
            r.load_weights(weights)
            r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], c.near, c.far, fr["support_fine"])
            ry = make_rays(c, fr)
            n = 96 - 17 * i
            o, d = torch.from_numpy(ry["rays_o"][:n]).to(dev), torch.from_numpy(ry["rays_d"][:n]).to(dev)
            qc = torch.from_numpy(fr["pose"][:3, 3])
            jobs.append((r, o, d, qc))
            if i == 1:   # a second job on the same frame, with per-ray centres
                jobs.append((r, o[:31], d[:31], (qc.to(dev)[None, :] + 0.01 * torch.arange(31, device=dev)[:, None]).contiguous()))
        want = [r.render_rays(o, d, qc) for r, o, d, qc in jobs]
        got = render_rays_multi(jobs)
        torch.cuda.synchronize()
        assert len(got) == len(want) == 5
        for a, b in zip(got, want):
            for k in b:
                assert torch.equal(a[k], b[k]), (prec, k)


def test_graphed_inference_replays_are_bit_identical_to_the_eager_call():
    """Round 5: `render_rays(graph=True)` replays a small batch shape as a HIP graph from the second call on (GraphedRender).  The replay must
    give the eager call's bits — for NEW rays, NEW depths and a NEW query centre fed through the same graph — in both parity modes, with and without explicit
    depths, and a frame / weight / precision change must drop the captured graph instead of replaying it against stale tables."""
    from nerf_loc_amd.renderer import GraphedRender
    from nerf_loc_amd.synth import make_frame
    sc = _scene("c1")
    cfg, frame, rays = sc["cfg"], sc["frame"], sc["rays"]
    for prec in ("f16mx", "bf16x3"):
        r = _renderer(sc, prec)
        t = torch.linspace(0, 1, cfg.S)
        z0 = (cfg.near * (1 - t) + cfg.far * t).expand(cfg.R, cfg.S).contiguous()
        qc = frame["pose"][:3, 3]
        for trial in range(4):
            sel = np.random.default_rng(trial).permutation(cfg.R)
            o, d = rays["rays_o"][sel], rays["rays_d"][sel]
            z = z0 * (1.0 + 0.01 * trial)
            q = qc + np.float32(0.01 * trial)
            eager = r.render_rays(o, d, q, z_vals=z)
            graphed = r.render_rays(o, d, q, z_vals=z, graph=True)
            if trial >= 1:
                assert isinstance(r._rgraphs[(cfg.R, False, True, True)], GraphedRender), "the second request of a shape captures the graph"
            for k in eager:
                assert torch.equal(eager[k], graphed[k]), (prec, trial, k)
        # depths left to the library (z_vals=None) are a different graph
        a = r.render_rays(rays["rays_o"], rays["rays_d"], qc)
        for _ in range(2):
            b = r.render_rays(rays["rays_o"], rays["rays_d"], qc, graph=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (prec, "no z", k)
        # a new frame drops the graphs: the replay must not run against the old tables
        fr2 = make_frame(cfg.replace(seed=cfg.seed + 50))
        r.set_frame(fr2["topk_images"], fr2["feat_fine_src"], fr2["vis_featmaps"], fr2["topk_Ks"], fr2["topk_poses"], cfg.near, cfg.far, fr2["support_fine"])
        e2 = r.render_rays(rays["rays_o"], rays["rays_d"], qc, z_vals=z0)
        for _ in range(3):
            g2 = r.render_rays(rays["rays_o"], rays["rays_d"], qc, z_vals=z0, graph=True)
        for k in e2:
            assert torch.equal(e2[k], g2[k]), (prec, "new frame", k)
        assert not torch.equal(e2["rgb"], eager["rgb"])


def test_precision_guard_at_the_boundary_checks_every_batch():
    """NL_RENDER_PRECISION_GUARD (ABI 7): the LIBRARY keeps a C-ABI caller / `HipRenderer` alone inside the validated range of its
    mode.  A frame whose feature maps are scaled until SOME rays score attention logits beyond f16mx's limit and others do not:
      * an unguarded render leaves the mode alone and reports the indicator;
      * a guarded render of the benign rays stays in f16mx (no escalation) — and the guarded render of the other rays, a LATER batch of the same frame, is
        re-rendered in the next mode (round 5's module-level guard looked at the first batch of a frame only); the outputs are bit-identical to rendering that
        batch in that mode directly and within 1e-4 of the fp32 mode; the frame then stays there (the benign rays now come out in the safer mode too);
      * a new frame starts from the configured mode."""
    import importlib.util
    import os
    from nerf_loc_amd import _lib as L
    from nerf_loc_amd.renderer import HipRenderer
    from nerf_loc_amd.synth import SceneConfig, make_frame, make_rays, make_weights
    spec = importlib.util.spec_from_file_location("scale_sweep", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "scale_sweep.py"))
    sweep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sweep)
    cfg = SceneConfig("guard_abi", R=48, S=32, W=128, V=4, H=48, Wimg=64, seed=31)
    base, rays, weights = make_frame(cfg), None, make_weights(cfg)
    rays = make_rays(cfg, base)
    limit = L.GUARD_LOGIT_LIMIT["f16mx"]
    z = _zbase(cfg, cfg.R)
    qc = base["pose"][:3, 3]

    def renderer(fr, prec="f16mx"):
        r = HipRenderer(cfg.W, cfg.C, cfg.S, prec)
        r.load_weights({k: torch.from_numpy(v) for k, v in weights.items()})
        r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])
        return r
    o, d = rays["rays_o"], rays["rays_d"]
    chosen, seen = None, []
    for fscale in [1.5 * (8.0 / 1.5) ** (i / 13.0) for i in range(14)]:   # |logit| grows about quadratically with the feature scale: find the scale that splits the batch
        fr = sweep.scaled_frame(base, fscale=fscale)
        per_ray = []
        for i in range(cfg.R):
            r = renderer(fr)    # (a fresh frame per ray: the indicator is cumulative per frame)
            r.render_rays(o[i:i + 1], d[i:i + 1], qc, z_vals=z[i:i + 1])
            per_ray.append(r.diagnostics()["logit_absmax"])
        per_ray = np.array(per_ray)
        benign, ill = np.where(per_ray < 0.97 * limit)[0], np.where(per_ray > 1.03 * limit)[0]
        seen.append((round(fscale, 3), float(per_ray.min()), float(np.median(per_ray)), float(per_ray.max()), len(benign), len(ill)))
        if per_ray.max() < L.GUARD_LOGIT_LIMIT["bf16x3"] and min(len(benign), len(ill)) >= 3 and (chosen is None or min(len(benign), len(ill)) > min(len(chosen[2]), len(chosen[3]))):
            chosen = (fscale, fr, benign, ill, per_ray)
    assert chosen is not None, ("no feature scale splits the rays around the f16mx limit: (scale, min, median, max, #below, #above)", seen)
    fscale, fr, benign, ill, per_ray = chosen
    print(f"feature scale {fscale:.3f}: {len(benign)} rays below {0.97 * limit:g}, {len(ill)} above {1.03 * limit:g} (min {per_ray.min():.1f}, max {per_ray.max():.1f})")
    zb, zi = z[:len(benign)], z[:len(ill)]
    # unguarded: nothing happens, the indicator is reported
    r = renderer(fr)
    plain = r.render_rays(o[ill], d[ill], qc, z_vals=zi)
    dg = r.diagnostics()
    assert dg["logit_absmax"] > limit and dg["guard_precision"] is None and dg["guard_escalations"] == 0
    # guarded, batch by batch against ONE frame
    r = renderer(fr)
    first = r.render_rays(o[benign], d[benign], qc, z_vals=zb, precision_guard=True)
    dg = r.diagnostics()
    assert dg["guard_precision"] == "f16mx" and dg["guard_escalations"] == 0 and dg["logit_absmax"] <= limit, dg
    second = r.render_rays(o[ill], d[ill], qc, z_vals=zi, precision_guard=True)
    dg = r.diagnostics()
    assert dg["guard_precision"] == "bf16x3" and dg["guard_escalations"] == 1, dg
    third = r.render_rays(o[benign], d[benign], qc, z_vals=zb, precision_guard=True)   # the frame stays in the safer mode
    assert r.diagnostics()["guard_escalations"] == 1 and r.diagnostics()["guard_precision"] == "bf16x3"
    rx = renderer(fr, "bf16x3")
    want_ill, want_benign = rx.render_rays(o[ill], d[ill], qc, z_vals=zi), rx.render_rays(o[benign], d[benign], qc, z_vals=zb)
    r32 = renderer(fr, "fp32")
    exact = r32.render_rays(o[ill], d[ill], qc, z_vals=zi)
    for k in KEYS:
        assert torch.equal(second[k], want_ill[k]) and torch.equal(third[k], want_benign[k]), k
        assert rel_err(second[k].cpu().numpy(), exact[k].cpu().numpy()) < 1e-4, (k, "guarded vs fp32 mode")
    assert not all(torch.equal(first[k], third[k]) for k in KEYS)    # (the first batch really was rendered in f16mx)
    assert not all(torch.equal(plain[k], second[k]) for k in KEYS)
    # a new frame starts from the configured mode; the guard is refused where it would serialise concurrent jobs
    r.set_frame(base["topk_images"], base["feat_fine_src"], base["vis_featmaps"], base["topk_Ks"], base["topk_poses"], cfg.near, cfg.far, base["support_fine"])
    r.render_rays(o, d, qc, z_vals=z, precision_guard=True)
    dg = r.diagnostics()
    assert dg["guard_precision"] == "f16mx" and dg["guard_escalations"] == 0 and 0 < dg["logit_absmax"] < limit
    # the staged kernels (W = 64: the v1 fused kernel; fp32 mode: the staged attention kernel) report the indicator too
    c64 = cfg.replace(W=64, name="guard_w64")
    w64 = make_weights(c64)
    for prec in ("bf16x3", "fp32"):
        r64 = HipRenderer(c64.W, c64.C, c64.S, prec)
        r64.load_weights({k: torch.from_numpy(v) for k, v in w64.items()})
        r64.set_frame(base["topk_images"], base["feat_fine_src"], base["vis_featmaps"], base["topk_Ks"], base["topk_poses"], cfg.near, cfg.far, base["support_fine"])
        r64.render_rays(o, d, qc, z_vals=z)
        assert r64.diagnostics()["logit_absmax"] > 0, prec
