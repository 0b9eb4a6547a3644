"""The density-head rungs (nerf_loc_amd.synth.SURFACE_RUNGS) make what they claim: scenes with surfaces, empty space and saturated
density on which the fp32 oracle is still a valid reference.  CPU only: the GPU tests of tests/test_gpu_surfaces.py render these scenes,
and this file keeps them from quietly degenerating into thin media again."""
import numpy as np
import pytest
import torch

from nerf_loc_amd.synth import SURFACE_RUNGS
from tests.golden_cases import build_case
from tests.util import OUT_KEYS, density_pre_activation, first_opaque, fp64_render, l2_rel, oracle_render, rel_err, surface_weights

CASE = "w256s128"


@pytest.fixture(scope="module")
def scene():
    case = build_case(CASE)
    return case, oracle_render(case, intermediates=True)


def test_the_unscaled_head_is_a_thin_medium(scene):
    """What the rungs exist for: with make_weights' own density head no ray is opaque before its last sample."""
    case, thin = scene
    pre = density_pre_activation(case["weights"], thin["geo"])
    assert abs(float(pre.mean()) + 0.7) < 0.2 and abs(float(pre.std()) - 0.56) < 0.15, (float(pre.mean()), float(pre.std()))
    assert int((first_opaque(thin["weights"]) < case["cfg"].S - 1).sum()) == 0


@pytest.mark.parametrize("rung", sorted(SURFACE_RUNGS))
def test_rung_scene_is_what_it_claims_and_the_oracle_is_a_valid_reference(scene, rung):
    """Rung A: every ray opaque (T < 1e-4) before sample S/2.  Rung C: at least a third of the rays opaque before their last sample, at least a third
    not before sample S/4, some pre-activation > 20 (softplus' linear branch) and at least 10 % < -10 (empty space).  Rung D: at least three
    quarters of the rays opaque, at least 5 % of the pre-activations > 20.  Every rung: the fp32 oracle within 1e-5 of the same function in
    fp64 on all five outputs, max-rel and L2-rel (a tenth of the 1e-4 the GPU tests apply, so the oracle is the reference there)."""
    case, thin = scene
    cfg = case["cfg"]
    R, S = cfg.R, cfg.S
    w, g, c = surface_weights(case, rung, thin)
    ref = oracle_render(case, w, intermediates=True)
    pre = density_pre_activation(w, ref["geo"])
    assert torch.equal(ref["geo"], thin["geo"]), "the density head is the only thing a rung changes"
    if SURFACE_RUNGS[rung] is not None:
        std, mean = SURFACE_RUNGS[rung]
        assert abs(float(pre.std()) - std) < 1e-3 * std and abs(float(pre.mean()) - mean) < 1e-3 * std, (float(pre.std()), float(pre.mean()))
    fo = first_opaque(ref["weights"])
    opaque = fo < S - 1          # T < 1e-4 in front of a sample before the last one
    hi, lo = float((pre > 20).float().mean()), float((pre < -10).float().mean())
    print(f"\nrung {rung}: g {g:.3f} c {c:+.3f}  pre std {float(pre.std()):.2f} mean {float(pre.mean()):+.2f} min {float(pre.min()):.1f} max {float(pre.max()):.1f}  "
          f"sigma {float(ref['sigma'].min()):.1e} ... {float(ref['sigma'].max()):.1f}  opaque {int(opaque.sum())}/{R}  first opaque "
          f"{int(fo.min())}/{int(fo.median())}/{int(fo.max())}  pre>20 {100 * hi:.1f} %  pre<-10 {100 * lo:.1f} %")
    if rung == "A":
        assert bool((fo < S // 2).all())
    if rung == "C":
        assert int(opaque.sum()) * 3 >= R and int((fo >= S // 4).sum()) * 3 >= R
        assert hi > 0 and lo >= 0.10
    if rung == "D":
        assert int(opaque.sum()) * 4 >= 3 * R and hi >= 0.05
    e64 = fp64_render(case, w)
    for k in OUT_KEYS:
        a, b = ref[k].numpy(), e64[k].numpy()
        print(f"    oracle fp32 vs fp64 {k:18s} max-rel {rel_err(a, b):.1e}  l2-rel {l2_rel(a, b):.1e}")
        assert rel_err(a, b) < 1e-5 and l2_rel(a, b) < 1e-5, (rung, k, rel_err(a, b), l2_rel(a, b))
    assert np.array_equal(ref["mask"].numpy(), e64["mask"].numpy())
