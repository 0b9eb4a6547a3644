"""Hierarchical sampling without a GPU: the fp64 restatement against the project's own eager code, the conditioning of every seeded recipe, the derived
tolerance against two independent fp32 evaluations (the oracle's, and an operation-by-operation emulation of sample_pdf_kernel), and the proof that the
assertions tests/test_gpu_hier.py makes on the GPU catch each one-line mutation of the kernels — shown here on the emulation, never by running a broken kernel."""
import functools

import numpy as np
import pytest
import torch

from tests import hier_cases as hc
from tests import hier_ref as hr

RESAMPLE = sorted(set(hc.ARITH_CASES) | {(sc, ni, r) for _, ni, sc, r in hc.MERGE_CASES})


@functools.lru_cache(maxsize=None)
def _case(key):
    case = hc.resample_case(*key)
    return case, hc.reference(case)


def test_restatement_equals_the_eager_code_in_double():
    """To 1e-12, plus the error model's own bound at the unit roundoff of double: numpy and torch round the total of a row differently (1e-16), and a sample in
    a bin of den ~ 1e-5 (1 - 2^-24 on `onehot_half`) turns that into 5e-12.  That term is below 1e-12 wherever den > 2e-4."""
    from nerf_loc_amd.diff_render import sample_pdf_diff
    worst = 0.0
    for key in RESAMPLE:
        case, ref = _case(key)
        t = lambda a: torch.from_numpy(np.asarray(a)).double()
        z = sample_pdf_diff(t(ref["bins"]), t(case["wc"][:, 1:-1]), t(case["u"])).numpy()
        worst = max(worst, float(np.abs(z - ref["z"]).max()))
        assert (np.abs(z - ref["z"]) <= 1e-12 + hr.tolerance(ref, ref["bins"], case["u"], unit=2.0 ** -53)).all(), key
    print(f"\n  restatement vs sample_pdf_diff in double: worst {worst:.1e}")


def test_every_sample_of_every_recipe_is_well_conditioned():
    for key in RESAMPLE:
        case, ref = _case(key)
        assert case["u"].dtype == np.float32 and (np.diff(case["u"], axis=1) >= 0).all() and (case["u"] >= 0).all() and (case["u"] < 1).all()
        assert ref["conditioned"].all(), (key, np.argwhere(~ref["conditioned"]).tolist())


def test_the_case_list_covers_what_the_gpu_test_asserts_on():
    rows_sc, rows_depth, specials = set(), set(), {"zero": 0, "top": 0, "collapsed_mid": 0}
    most, fewest = 0.0, 1.0
    for key in RESAMPLE:
        case, ref = _case(key)
        collapsed, uncertain = hr.bin_classes(ref)
        nb = collapsed.shape[1]
        for r in range(case["R"]):
            rows_sc.add((case["rows"][r], case["Sc"]))
            rows_depth.add((case["rows"][r], case["depths"][r]))
            most, fewest = max(most, collapsed[r].sum() / nb), min(fewest, collapsed[r].sum() / nb)
            k = np.minimum(ref["lo"][r], nb - 1)
            specials["zero"] += int((case["u"][r] == 0).sum())
            specials["top"] += int((case["u"][r] == np.float32(1 - 2.0 ** -24)).sum())
            specials["collapsed_mid"] += int(collapsed[r][k].sum())
    assert rows_sc == {(n, s) for n in hc.WEIGHT_ROWS for s in hc.SC}
    assert rows_depth == {(n, d) for n in hc.WEIGHT_ROWS for d in hc.DEPTH_ROWS}
    assert most > 0.5 and fewest == 0.0, "a ray with more than nb / 2 collapsed bins, and one with none"
    assert all(v >= 10 for v in specials.values()), specials
    assert {r for _, _, r in hc.ARITH_CASES} == set(hc.RS) and {(sc, ni) for sc, ni, _ in hc.ARITH_CASES} == {(s, n) for s in hc.SC for n in hc.NI}
    assert any(sb + ni == 256 for sb, ni, _, _ in hc.MERGE_CASES)


def test_zeros_rows_follow_the_closed_form():
    seen = 0
    for key in RESAMPLE:
        case, ref = _case(key)
        closed = hc.zeros_closed_form(case)
        for r, name in enumerate(case["rows"]):
            if name == "zeros":
                seen += 1
                assert np.abs(closed[r] - ref["z"][r]).max() < 1e-12 * hc.FAR
    assert seen >= 5


def test_the_fp32_oracle_meets_the_tolerance_on_every_recipe():
    from oracle.render_oracle import sample_pdf
    worst = 0.0
    for key in RESAMPLE:
        case, ref = _case(key)
        t = torch.from_numpy
        z = sample_pdf(t(ref["bins"]), t(case["wc"][:, 1:-1].copy()), case["Ni"], t(case["u"])).numpy()
        z_out = np.concatenate([np.sort(z, 1), hc.above_far(case["R"])], 1)
        assert not hc.arith_failures(case, ref, z_out), (key, hc.arith_failures(case, ref, z_out)[:4])
        worst = max(worst, float((np.abs(z - ref["z"]) / (hc.FAR - hc.NEAR)).max()))
    print(f"\n  fp32 oracle vs fp64 restatement: worst error {worst:.1e} of the depth range")


def _emulate(case, zb, mutation=None):
    return hr.sample_pdf_kernel32(case["zc"], case["wc"], case["u"], zb, mutation)


def test_the_kernel_emulation_meets_the_tolerance_and_merges_exactly():
    """sample_pdf_kernel's arithmetic in fp32 on the CPU passes every assertion of the GPU stage test: the tolerance is not too tight for a correct kernel."""
    worst = 0.0
    for key in RESAMPLE:
        case, ref = _case(key)
        z_out = _emulate(case, hc.above_far(case["R"]))
        assert not hc.arith_failures(case, ref, z_out), (key, hc.arith_failures(case, ref, z_out)[:4])
        worst = max(worst, float((np.abs(z_out[:, :-1] - ref["z"]) / (hc.FAR - hc.NEAR)).max()))
    print(f"\n  fp32 kernel emulation vs fp64 restatement: worst error {worst:.1e} of the depth range")
    for sb, ni, sc, r in hc.MERGE_CASES:
        case, _ = _case((sc, ni, r))
        zb = hc.base_rows(case, sb)
        zf = _emulate(case, hc.above_far(r))[:, :ni]
        assert not hc.merge_failures(zb, zf, _emulate(case, zb))


@pytest.mark.parametrize("mutation", hr.MUTATIONS)
def test_each_mutation_of_the_resampling_kernel_fails_a_stage_assertion(mutation):
    """den < eps dropped; `above` clamped to nb - 1; cdf inclusive instead of exclusive; sort padding 0: the emulation with that one line changed must fail
    the arithmetic or the merge assertion on at least one case of the list the GPU test runs."""
    caught = []
    for key in hc.ARITH_CASES:
        case, ref = _case(key)
        if hc.arith_failures(case, ref, _emulate(case, hc.above_far(case["R"]), mutation)):
            caught.append(("arith", key))
    for sb, ni, sc, r in hc.MERGE_CASES:
        case, _ = _case((sc, ni, r))
        zb = hc.base_rows(case, sb)
        zf = _emulate(case, hc.above_far(r))[:, :ni]      # the unmutated samples: only the merge is on trial
        if hc.merge_failures(zb, zf, _emulate(case, zb, mutation)):
            caught.append(("merge", (sb, ni)))
    print(f"\n  {mutation}: caught by {len(caught)} cases, e.g. {caught[:3]}")
    assert caught
    if mutation == "pad_zero":
        assert {c[0] for c in caught} >= {"merge"} and ("merge", (64, 192)) not in caught, "a full network has no padding"


def test_a_ray_no_view_sees_goes_to_the_ground_state_and_the_mutation_shows():
    """coarse_ray_kernel with `nmask == 0` ignored gives alpha = 0 / 1e-8 = 0 -> sigmoid = 0.5 on an unseen sample; the off-view assertion of the GPU test
    (weights == ground_weights within the bar) then fails by ~0.5."""
    V, R, Sc = 3, 2, 13
    z = np.zeros((V, R, Sc))
    good = hr.coarse_ray64(z, z, z)
    assert np.abs(good - hr.ground_weights(Sc)).max() < 1e-15
    bad = hr.coarse_ray64(z, z, z, ignore_nmask=True)
    assert np.abs(bad - hr.ground_weights(Sc)).max() > 0.4


# ----------------------------------------------------------------------------- coarse-weight scenes: conditions on the inputs of the GPU test
def test_coarse_scenes_keep_clear_of_mask_edges_and_hold_opaque_and_unseen_rays():
    """For every scene tests/test_gpu_hier.py runs: no sample projects within 1e-3 px of a view's border or within 1e-3 of a camera plane (fp64 projection), so
    the in-view mask is the same in every arithmetic; the rays through OFF_PIX are seen by no view; the sharpened `hier` decoders give opaque rays."""
    opaque = 0
    for name, V, (R, Sc), jitter, off_block in hc.COARSE_SCENES:
        sc = hc.coarse_scene(name, V, R, Sc, jitter, off_block=off_block)
        px, py, dep, mask = hr.coarse_projection64(sc["frame"], sc["pix"], sc["K"], sc["pose"], sc["zc"])
        margin, dmin = hr.border_margin(sc["frame"], px, py, dep)
        assert margin > 1e-3 and dmin > 1e-3, (name, V, R, Sc, jitter, margin, dmin)
        assert not mask[:, sc["off"]].any() and sc["off"].sum() == off_block
        assert mask[:, ~sc["off"]].any(), "some ray is seen"
        if name == "hier":
            w = hc.coarse_weights_ref(sc, hc.sharpened(sc["weights"]), torch.float64)
            opaque += int(((w.sum(1) > 0.999) & (w.max(1) > 0.9)).sum())
    assert opaque >= 5, opaque
    # 63 consecutive unseen rows hold a whole 32-row tile of the MFMA kernel wherever they start: its early-out runs, between tiles that are seen
    assert any(off * shape[1] >= 63 for _, _, shape, _, off in hc.COARSE_SCENES)


def test_the_chain_draws_are_well_conditioned_on_the_reference_weights_and_meet_collapsed_bins():
    """tests/test_gpu_hier.py asserts the conditioning of the chain's draws on the KERNEL's coarse weights; the seeds are chosen here, on the reference's, in
    double and in single precision, with every draw at least 2e-5 from the upper knot of a collapsed or undecidable bin."""
    sc = hc.chain_case()
    bins = hr.mid_points32(sc["zc"])
    for dtype in (torch.float64, torch.float32):
        w = hc.coarse_weights_ref(sc, sc["weights"], dtype).astype(np.float32)
        for Ni in hc.CHAIN_NI:
            u = hc.chain_u(Ni, len(w))
            ref = hr.sample_pdf64(bins, w[:, 1:-1], u)
            collapsed, uncertain = hr.bin_classes(ref)
            assert hr.conditioned(ref, u).all(), (dtype, Ni)
            d = np.abs(u[:, :, None].astype(np.float64) - ref["cdf"][:, None, 1:])
            assert np.where((collapsed | uncertain)[:, None, :], d, 1.0).min() > 2e-5
            assert (collapsed.sum(1) > collapsed.shape[1] // 2).any() and (collapsed.sum(1) == 0).any()
