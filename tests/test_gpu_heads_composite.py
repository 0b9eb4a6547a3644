"""nl_heads_composite (rows a14-a18 as a stage: density head, colour-blend tail, feat_mlp, front-to-back compositing, valid-ray mask) on its own,
against conditional_nerf/model.py:525-597 restated in fp64 torch on the CPU right here, driven to the edges directly (run with `pytest -m gpu`).

The density is steered through `geo`: for a target pre-activation t_n, geo[n] = (t_n - b) w / |w|^2 plus a component orthogonal to w, so any sigma
profile can be fed without touching the weights.  Every composite_kernel<CH> instance (S <= 64, 128, 192, 256), both branches of nl_softplus, an alpha
that rounds to 1, underflowing transmittance, empty space, repeated depths and a partly filled workgroup are reached with an fp64 reference on the
other side."""
import ctypes as ct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_loc_amd import diff_render as dr
from nerf_loc_amd.synth import SceneConfig, make_weights
from tests.util import l2_rel, rel_err

pytestmark = pytest.mark.gpu

V = 5
PROFILES = ("thin", "step", "softplus", "empty_then_last", "empty", "generator", "generator_x40", "repeated_z", "wide")


def _targets(profile, S, g):
    """-> (z (S,), target density pre-activation t (S,)) of one ray, fp64"""
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inv_softplus = lambda x: torch.where(x > 30, x, torch.log(torch.expm1(x.clamp(max=30.0)).clamp(min=1e-300)))
    z = 0.3 + (4.7 / S) * torch.arange(S, dtype=torch.float64)
    if profile == "thin":                 # alpha ~ 0.03 per sample, opaque through the last 1e2 interval only
        t = -0.7 + 0.56 * rnd(S)
    elif profile == "step":               # empty space, then sigma ~ 50 at 0.5 spacing: alpha rounds to exactly 1 in fp32 (exp(-25) < 2^-25), T = 0 behind it
        z = 0.3 + 0.5 * torch.arange(S, dtype=torch.float64)
        t = torch.where(torch.arange(S) < S // 3, torch.full((S,), -30.0, dtype=torch.float64), 50.0 + rnd(S))
    elif profile == "softplus":           # around nl_softplus' switch to its linear branch; spacing 0.02 keeps alpha away from 1 so that sigma is visible in the weights
        z = 0.3 + 0.02 * torch.arange(S, dtype=torch.float64)
        t = torch.tensor([20.0, 20.0 - 1e-3, 20.0 + 1e-3, 80.0, 19.0, 21.0, 20.0 - 1e-5, 20.0 + 1e-5], dtype=torch.float64).repeat(S // 8 + 1)[:S]
    elif profile == "empty_then_last":    # weights all ~ 0 but the last: sum(weights) reaches 1 only through the last 1e2 interval
        t = torch.full((S,), -60.0, dtype=torch.float64)
        t[-1] = 5.0
    elif profile == "empty":              # nothing at all: sigma = 9e-27 everywhere, sum(weights) ~ 1e-24, white_bkgd leaves rgb = 1
        t = torch.full((S,), -60.0, dtype=torch.float64)
    elif profile in ("generator", "generator_x40"):   # test_backward_kernels._composite_inputs: "thin to opaque, some rays saturate (T underflows behind them)"
        z = torch.sort(0.3 + 4.7 * torch.rand(S, generator=g, dtype=torch.float64))[0]
        t = inv_softplus(F.softplus(2 * rnd(S)) * (40.0 if profile.endswith("x40") else 1.0))
    elif profile == "repeated_z":         # delta = 0 (as the hierarchical merge of coarse and resampled depths produces), density thin to dense
        z = torch.sort(0.3 + 4.7 * torch.rand(S, generator=g, dtype=torch.float64))[0]
        z[1::3] = z[0:-1:3][: len(z[1::3])]
        t = 1.0 + 3.0 * rnd(S)
    else:                                 # "wide": rung D of the surface scenes (std 15, mean 0): 1e-20 ... 60
        t = 15.0 * rnd(S)
    return z, t


def _inputs(S, R, C, W, seed, weights):
    """-> fp32 CPU tensors z (R,S), fa, geo (R*S,W), bl1 (R*S,V,32), rgbv (R*S,V,4), valid_s (R*S) int32; profile of ray r = PROFILES[(r + seed) % 9]"""
    g = torch.Generator().manual_seed(1000 * S + 10 * R + seed)
    w = torch.from_numpy(weights["sigma_mlp.0.weight"]).double().view(-1)
    b = float(weights["sigma_mlp.0.bias"][0])
    zs, ts, names = [], [], []
    for r in range(R):
        names.append(PROFILES[(r + seed) % len(PROFILES)])
        z, t = _targets(names[-1], S, g)
        zs.append(z); ts.append(t)
    z, t = torch.stack(zs), torch.stack(ts).view(-1)
    N = R * S
    orth = 0.5 * torch.randn(N, W, generator=g, dtype=torch.float64)
    orth = orth - (orth @ w)[:, None] * w[None] / (w @ w)
    geo = ((t - b)[:, None] * w[None] / (w @ w) + orth).float()
    fa = torch.randn(N, W, generator=g)
    bl1 = 0.5 * torch.randn(N, V, 32, generator=g)
    rgbv = torch.rand(N, V, 4, generator=g)
    rgbv[..., 3] = torch.where(torch.rand(N, V, generator=g) < 0.3, torch.zeros(N, V), rgbv[..., 3])    # invisible views: masked_fill(-1e9)
    rgbv[::11, :, 3] = 0.0                                                                              # samples no view sees: uniform softmax
    # valid samples per ray: 0, 8 (mask False: the rule is `> 8`), 9 (True) and random shares
    valid = (torch.rand(R, S, generator=g) < torch.rand(R, 1, generator=g)).int()
    for r, n in zip(range(R), (0, 8, 9)):
        valid[r] = 0
        valid[r, torch.randperm(S, generator=g)[: min(n, S)]] = 1
    return z.float(), fa, geo, bl1, rgbv, valid.view(-1).contiguous(), names


def _reference(weights, z, fa, geo, bl1, rgbv, valid_s, white, dtype=torch.float64):
    """conditional_nerf/model.py:525-597 in plain torch on the CPU: softplus density head, blend tail (layer 1 split by linearity as the entry point takes it:
    feature_agg's columns here, the per-(sample, view) part = bl1), feat_mlp, composite, mask rule `> 8` valid samples.
    -> (outputs dict, sigma (R,S), rgb_s, ft): the last three so that the SAME compositing inputs can be run through the fp32 eager expression"""
    p = {k: torch.from_numpy(v).to(dtype) for k, v in weights.items()}
    z, fa, geo, bl1, rgbv = (t.to(dtype) for t in (z, fa, geo, bl1, rgbv))
    R, S = z.shape
    W = fa.shape[1]
    lrelu = lambda x: F.leaky_relu(x, 0.01)
    pre = F.linear(geo, p["sigma_mlp.0.weight"], p["sigma_mlp.0.bias"]).view(R, S)
    sigma = torch.logaddexp(pre, torch.zeros_like(pre))          # softplus without a threshold
    x = lrelu(F.linear(fa, p["rgb_blending_mlp.0.weight"][:, :W]).unsqueeze(1) + bl1)
    x = lrelu(F.linear(x, p["rgb_blending_mlp.2.weight"], p["rgb_blending_mlp.2.bias"]))
    lg = F.linear(x, p["rgb_blending_mlp.4.weight"], p["rgb_blending_mlp.4.bias"])
    bw = F.softmax(lg.masked_fill(rgbv[..., 3:4] == 0, -1e9), dim=1)
    rgb_s = (rgbv[..., :3] * bw).sum(1).view(R, S, 3)
    ft = F.linear(lrelu(F.linear(fa, p["feat_mlp.0.weight"], p["feat_mlp.0.bias"])), p["feat_mlp.2.weight"], p["feat_mlp.2.bias"]).view(R, S, -1)
    # composite (model.py:544-560, 597), restated here so that the reference shares no code with the project
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e2)], -1)
    alpha = 1 - torch.exp(-delta * sigma)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], -1), -1)      # exclusive product
    wts = alpha * T
    rgb = (wts[..., None] * rgb_s).sum(1) + ((1 - wts.sum(1))[:, None] if white else 0.0)
    depth = (wts * z).sum(1)
    unc = (wts * (z - depth[:, None]) ** 2).sum(1)
    feat = (wts[..., None] * ft).sum(1)
    out = {"rgb": rgb, "depth": depth, "depth_uncertainty": unc, "feat": feat, "weights": wts, "mask": valid_s.view(R, S).sum(1) > 8}
    return out, sigma, rgb_s, ft


_RENDERERS = {}


def _renderer(S, C, W, precision="fp32"):
    """one HipRenderer per S (the ray U-Net's LayerNorm tables bake S in); no frame: the entry point needs the packed weights only"""
    from nerf_loc_amd.renderer import HipRenderer
    key = (S, C, W)
    if key not in _RENDERERS:
        weights = make_weights(SceneConfig("heads", S=S, W=W, C=C, seed=31))
        r = HipRenderer(W, C, S, precision)
        r.load_weights({k: torch.from_numpy(v) for k, v in weights.items()})
        _RENDERERS[key] = (r, weights)
    r, weights = _RENDERERS[key]
    r.set_precision(precision)
    return r, weights


def _check(S, R, C, W, white, want_weights, want_feat, seed, precision="fp32"):
    r, weights = _renderer(S, C, W, precision)
    z, fa, geo, bl1, rgbv, valid_s, names = _inputs(S, R, C, W, seed, weights)
    out = r.heads_composite(z, fa, geo, bl1, rgbv, valid_s, white, want_weights=want_weights, want_feat=want_feat, want_sigma=True)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    assert ("weights" in out) == want_weights and ("feat" in out) == want_feat
    ref, sigma, rgb_s, ft = _reference(weights, z, fa, geo, bl1, rgbv, valid_s, white)
    # the bar: as close to fp64 as the fp32 eager expression is on the same compositing inputs, 2e-6 where that is within a third of it
    e32 = dict(zip(("rgb", "depth", "depth_uncertainty", "feat", "weights"), dr.composite_eager(sigma.float(), rgb_s.float(), ft.float(), z, white)))
    tag = f"S={S} R={R} C={C} white={int(white)} weights={int(want_weights)} feat={int(want_feat)} {precision} [{names[0]}..]"
    line, fails = [], []
    for k in ("weights", "depth", "depth_uncertainty", "rgb"):
        if k not in out:
            continue
        assert torch.isfinite(out[k]).all(), (tag, k)
        e_hip, e_ref = rel_err(out[k].numpy(), ref[k].numpy()), rel_err(e32[k].numpy(), ref[k].numpy())
        bar = max(2e-6, 3 * e_ref)
        if k == "rgb" and precision != "fp32":
            bar = max(bar, 1e-4)      # rgb_s comes out of the blend projection, a split-bf16 product in this mode: the mode's own bar
        line.append(f"{k} {e_hip:.1e} (eager fp32 {e_ref:.1e})")
        if not e_hip < bar:
            fails.append((k, e_hip, "bar", bar))
    if want_feat:
        # feat_mlp runs as two matrix products of the mode: the mode's published bar (5e-5 fp32, 1e-4 bf16x3), max-rel and L2-rel
        assert torch.isfinite(out["feat"]).all(), tag
        bar = 5e-5 if precision == "fp32" else 1e-4
        e, l2 = rel_err(out["feat"].numpy(), ref["feat"].numpy()), l2_rel(out["feat"].numpy(), ref["feat"].numpy())
        line.append(f"feat {e:.1e}/{l2:.1e}")
        if not (e < bar and l2 < bar):
            fails.append(("feat", e, l2, "bar", bar))
    # per-sample density, both softplus branches: relative to the sample's own value where the head saturates, the pre-activation's rounding below that
    sg, pre = out["sigma"].double(), torch.log(torch.expm1(sigma.clamp(max=30.0)).clamp(min=1e-300)).where(sigma <= 30, sigma)
    bound = 4e-6 * (1 + pre.abs()) * torch.sigmoid(pre) + 1e-37     # |d pre| <= 4e-6 (1 + |pre|): a 256-term fp32 dot product whose terms sum to ~|pre| + 1
    e_sig = float(((sg - sigma).abs() / bound).max())
    line.append(f"sigma/bound {e_sig:.2f}")
    if not e_sig <= 1.0:
        fails.append(("sigma", e_sig))
    print(f"  {tag}: " + "  ".join(line))
    assert not fails, (tag, fails)
    assert torch.equal(out["mask"], ref["mask"]), tag
    if want_weights:
        w = out["weights"].double()
        assert float((w.sum(1) - ref["weights"].sum(1)).abs().max()) < 1e-6, tag
        opaque = (ref["weights"].sum(1) - 1).abs() < 1e-9
        assert float((w.sum(1)[opaque] - 1).abs().max() if bool(opaque.any()) else 0.0) < 1e-6, tag
        # behind an alpha that rounds to 1 in fp32 (delta * sigma >= 20: exp(-20) = 2e-9 < 2^-25) the transmittance is exactly 0, and so is every later weight
        delta = torch.cat([z[:, 1:].double() - z[:, :-1].double(), torch.full((R, 1), 1e2, dtype=torch.float64)], 1)
        sat = (delta * sigma >= 20.0)
        behind = (torch.cumsum(sat.int(), 1) - sat.int()) > 0
        assert bool((out["weights"][behind] == 0).all()), (tag, "weights behind an alpha of exactly 1 must be exactly 0")
        assert "step" not in names or int(behind.sum()) > 0, "the step profile is there to reach this"
    return out


@pytest.mark.parametrize("R", [1, 3, 5, 37])
@pytest.mark.parametrize("S", [8, 40, 64, 128, 192, 256])
def test_heads_composite_matches_fp64(S, R):
    """Every composite_kernel<CH> instance (CH = 1: S = 8, 40, 64; 2: 128; 3: 192; 4: 256; S not a multiple of 64 included), R = 1 ... 37 (partly filled
    workgroup of four waves), C in {7, 192}, white_bkgd both ways, out.weights null and non-null, out.feat null — each combination of S and R runs
    four calls that between them take every value of the other switches, with the ray profiles rotated so that small R meet every profile too."""
    i = [8, 40, 64, 128, 192, 256].index(S) * 4 + [1, 3, 5, 37].index(R)
    print()
    for j, (white, want_w, want_f) in enumerate([(False, True, True), (True, False, True), (True, True, False), (False, False, False)]):
        C, W = ((7, 64), (192, 256))[(i + j) % 2]
        _check(S, R, C, W, white, want_w, want_f, seed=i * 4 + j)


@pytest.mark.parametrize("S", [64, 128])
def test_heads_composite_in_the_split_bf16_mode(S):
    """The same entry point in bf16x3 (f16mx runs as bf16x3 outside the fused render path): the blend projection and feat_mlp are split-bf16 products there
    (rgb / feat at the mode's 1e-4); density head and compositing are fp32 kernels in every mode and keep their bars."""
    print()
    for seed, white in ((0, False), (4, True)):
        _check(S, 37, 192, 256, white, True, True, seed=seed, precision="bf16x3")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_heads_composite_after_mv_aggregate_matches_oracle_on_a_scene_with_surfaces(precision):
    """The staged hand-over as a caller would make it: nl_mv_aggregate's blend1 / rgbv / valid_s (`mv_aggregate(want_blend=True)`) and the oracle's feature_agg / geo
    into nl_heads_composite, on golden scene w256s128 with the density head of rung C (surfaces, empty space, both softplus branches), against the oracle's
    render at the mode's bar — which also pins the layout of the three per-view inputs the synthetic cases above assume."""
    from tests.golden_cases import build_case
    from tests.util import OUT_KEYS, oracle_render, surface_weights
    from nerf_loc_amd.renderer import HipRenderer
    from oracle.render_oracle import sample_depths
    case = build_case("w256s128")
    cfg, fr, rays = case["cfg"], case["frame"], case["rays"]
    w, _, _ = surface_weights(case, "C")
    ref = oracle_render(case, w, intermediates=True)
    r = HipRenderer(cfg.W, cfg.C, cfg.S, precision)
    r.load_weights({k: torch.from_numpy(v) for k, v in w.items()})
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])
    z = sample_depths(cfg.S, torch.tensor(cfg.near), torch.tensor(cfg.far)).expand(cfg.R, cfg.S).contiguous()
    zo, xyz = r.sample_points(rays["rays_o"], rays["rays_d"], z)
    _, valid_s, bl1, rgbv = r.mv_aggregate(xyz, fr["pose"][:3, 3], want_blend=True)
    assert tuple(bl1.shape) == (cfg.R * cfg.S, cfg.V, 32) and tuple(rgbv.shape) == (cfg.R * cfg.S, cfg.V, 4)
    out = r.heads_composite(zo, ref["feature_agg"], ref["geo"], bl1, rgbv, valid_s, False, want_sigma=True)
    torch.cuda.synchronize()
    bar = 5e-5 if precision == "fp32" else 1e-4
    assert np.array_equal(out["mask"].cpu().numpy(), ref["mask"].numpy())
    errs = {k: (rel_err(out[k].cpu().numpy(), ref[k].numpy()), l2_rel(out[k].cpu().numpy(), ref[k].numpy())) for k in OUT_KEYS + ("sigma",)}
    print("\n  heads_composite after mv_aggregate, w256s128 rung C, " + precision + ": " + "  ".join(f"{k} {a:.1e}/{b:.1e}" for k, (a, b) in errs.items()))
    assert all(a < bar and b < bar for a, b in errs.values()), errs


def test_heads_composite_validates_its_arguments():
    """The status codes the entry point returns today, so that they cannot change unnoticed: NL_OK for an empty batch (pointers may be null), NL_ERR_BAD_ARG for a
    null `out` / input / negative R / view count outside 1 ... NL_MAX_VIEWS, NL_ERR_WORKSPACE for a workspace below nl_heads_composite_workspace_bytes,
    NL_ERR_UNSUPPORTED for S = 264 (a configuration but for its size: more than composite_kernel's four samples per lane, nothing is launched)."""
    from nerf_loc_amd import _lib as L
    S, R, C, W = 40, 3, 7, 64
    r, weights = _renderer(S, C, W)
    z, fa, geo, bl1, rgbv, valid_s, _ = _inputs(S, R, C, W, 0, weights)
    dev = r.device
    z, fa, geo, bl1, rgbv, valid_s = (t.to(dev) for t in (z, fa, geo, bl1, rgbv, valid_s))
    outs = {"rgb": torch.zeros(R, 3, device=dev), "depth": torch.zeros(R, device=dev), "weights": torch.zeros(R, S, device=dev)}
    ro = L.NlRenderOut()
    for k, t in outs.items():
        setattr(ro, k, t.data_ptr())
    need = r.lib.nl_heads_composite_workspace_bytes(ct.byref(r.cfg), V, R)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(cfg=r.cfg, packed=r.packed.data_ptr(), v=V, zp=z.data_ptr(), out=ct.byref(ro), R_=R, wsp=ws.data_ptr(), nbytes=need, b1=bl1.data_ptr()):
        return r.lib.nl_heads_composite(ct.byref(cfg), packed, v, zp, fa.data_ptr(), geo.data_ptr(), b1, rgbv.data_ptr(), valid_s.data_ptr(), R_, 0, out, wsp, nbytes, st)
    assert call() == L.NL_OK
    torch.cuda.synchronize()
    assert float(outs["weights"].sum()) > 0
    assert call(R_=0, zp=None, out=None, wsp=None, nbytes=0) == L.NL_OK
    assert call(out=None) == L.NL_ERR_BAD_ARG
    assert call(zp=None) == L.NL_ERR_BAD_ARG
    assert call(b1=None) == L.NL_ERR_BAD_ARG
    assert call(packed=None) == L.NL_ERR_BAD_ARG
    assert call(wsp=None) == L.NL_ERR_BAD_ARG
    assert call(R_=-1) == L.NL_ERR_BAD_ARG
    assert call(v=0) == L.NL_ERR_BAD_ARG and call(v=L.MAX_VIEWS + 1) == L.NL_ERR_BAD_ARG
    assert call(nbytes=need - 1) == L.NL_ERR_WORKSPACE
    assert call(cfg=L.NlConfig(W, C, 264, L.PREC_F32)) == L.NL_ERR_UNSUPPORTED
    assert call(cfg=L.NlConfig(W, C, 260, L.PREC_F32)) == L.NL_ERR_BAD_ARG       # not a configuration at all, like S = 36 below
    assert call(cfg=L.NlConfig(W, C, 36, L.PREC_F32)) == L.NL_ERR_BAD_ARG        # S not a multiple of 8: not a configuration at all
    assert r.lib.nl_heads_composite_workspace_bytes(ct.byref(L.NlConfig(W, C, 264, L.PREC_F32)), V, R) == 0
    torch.cuda.synchronize()
