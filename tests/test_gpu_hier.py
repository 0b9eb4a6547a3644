"""Stage tests of hierarchical sampling on the GPU (csrc/hier.hip; run with `pytest -m gpu -s` to see the measured errors): nl_sample_pdf and
nl_coarse_weights called directly through ctypes, as nerf_loc_amd/renderer.py calls them, and the chain of the two on a scene with opaque rays.

Resampling is held per sample to the tolerance derived in tests/hier_ref.py against its fp64 restatement, on recipes (tests/hier_cases.py) every sample of
which is well-conditioned (tests/test_hier_cpu.py asserts that, and shows on a CPU emulation that these assertions catch each one-line mutation of the kernel);
the merge is held bit for bit.  The coarse weights are held to max(2e-5, 3 x the deviation of the eager restatement in fp32 from itself in fp64) of the
largest weight, per scene, computed from the reference alone.  Output buffers are poisoned with NaN before every call."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from tests import hier_cases as hc
from tests import hier_ref as hr
from tests.util import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("fp32", "bf16x3", "bf16", "f16mx")     # every precision the library takes: fp32 runs coarse_view_kernel, the others coarse_view_mfma_kernel


def _L():
    from nerf_loc_amd import _lib as L
    return L, L.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _sample_pdf(zc, wc, u, zb):
    """nl_sample_pdf on the current stream -> z_out (R, Sb + Ni) numpy; the output starts as NaN."""
    L, lib = _L()
    R, Sc = zc.shape
    Ni, Sb = u.shape[1], zb.shape[1]
    d = [_dev(a) for a in (zc, wc, u, zb)]
    out = torch.full((R, Sb + Ni), float("nan"), device=DEV)
    L.check(lib.nl_sample_pdf(d[0].data_ptr(), d[1].data_ptr(), Sc, d[2].data_ptr(), Ni, d[3].data_ptr(), Sb, R, out.data_ptr(),
                              torch.cuda.current_stream().cuda_stream), "nl_sample_pdf")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(key):
    case = hc.resample_case(*key)
    return case, hc.reference(case)


# ----------------------------------------------------------------------------- nl_sample_pdf
@pytest.mark.parametrize("Sc,Ni,R", hc.ARITH_CASES)
def test_resampled_depths_match_fp64_per_sample(Sc, Ni, R):
    """Sb = 1 with the base depth beyond the far plane: output position i is sample i.  Every sample within hier_ref.tolerance of sample_pdf64, `zeros` rows
    within it of the closed form too; the second call gives the same bits."""
    case, ref = _case((Sc, Ni, R))
    assert ref["conditioned"].all()
    z = _sample_pdf(case["zc"], case["wc"], case["u"], hc.above_far(R))
    err = np.abs(z[:, :Ni] - ref["z"])
    worst = np.unravel_index(np.argmax(err / ref["tolerance"]), err.shape)
    print(f"\n  Sc {Sc:2d} Ni {Ni:3d} R {R}: worst error / tolerance {float((err / ref['tolerance']).max()):.3f} (ray {worst[0]} `{case['rows'][worst[0]]}`, "
          f"error {err[worst]:.2e}, tolerance {ref['tolerance'][worst]:.2e}); largest error {err.max() / (hc.FAR - hc.NEAR):.1e} of the range")
    fails = hc.arith_failures(case, ref, z)
    assert not fails, fails[:8]
    again = _sample_pdf(case["zc"], case["wc"], case["u"], hc.above_far(R))
    assert np.array_equal(z.view(np.uint32), again.view(np.uint32)), "two calls, the same bits"


@pytest.mark.parametrize("Sb,Ni,Sc,R", hc.MERGE_CASES)
def test_merge_with_the_base_depths_is_exact(Sb, Ni, Sc, R):
    """The output is np.sort(concat(z_base, zf)) bit for bit, zf being the kernel's own samples (from the Sb = 1 call): the bitonic network and its padding,
    with base rows that hold byte-copies of bin mid-points, duplicates and depths outside [near, far].  Sb + Ni = 256 leaves no padding at all."""
    case, ref = _case((Sc, Ni, R))
    first = _sample_pdf(case["zc"], case["wc"], case["u"], hc.above_far(R))
    assert not hc.arith_failures(case, ref, first)
    zb = hc.base_rows(case, Sb)
    z = _sample_pdf(case["zc"], case["wc"], case["u"], zb)
    fails = hc.merge_failures(zb, first[:, :Ni], z)
    assert not fails, fails[:8]
    assert np.array_equal(z.view(np.uint32), _sample_pdf(case["zc"], case["wc"], case["u"], zb).view(np.uint32))


@pytest.mark.parametrize("Sc,Ni,Sb", [(64, 65, 1), (5, 7, 3), (33, 192, 64)])
def test_a_ray_does_not_depend_on_the_rays_of_its_workgroup(Sc, Ni, Sb):
    """Four rays share a workgroup and its LDS: every ray of a 9-ray batch gives the bits it gives alone (R = 1)."""
    case, _ = _case((Sc, Ni, 9))
    zb = hc.base_rows(case, Sb)
    full = _sample_pdf(case["zc"], case["wc"], case["u"], zb)
    for r in range(9):
        alone = _sample_pdf(case["zc"][r:r + 1], case["wc"][r:r + 1], case["u"][r:r + 1], zb[r:r + 1])
        assert np.array_equal(full[r].view(np.uint32), alone[0].view(np.uint32)), r


def test_entry_points_reject_shapes_outside_their_contract():
    """include/nerfloc_render.h: nl_sample_pdf answers Sb < 0, Ni < 1, Sb + Ni < 1, Sc < 3 with NL_ERR_BAD_ARG and Sb + Ni > 256, Sc > 64 with
    NL_ERR_UNSUPPORTED, before any launch (the output stays NaN); nl_coarse_weights judges Sc before it looks at the workspace."""
    L, lib = _L()
    buf = torch.zeros(4 * 300, device=DEV)
    out = torch.full((4 * 300,), float("nan"), device=DEV)
    p, o = buf.data_ptr(), out.data_ptr()
    call = lambda Sc, Ni, Sb, R=4: lib.nl_sample_pdf(p, p, Sc, p, Ni, p, Sb, R, o, None)
    for Sc, Ni, Sb in [(64, 16, -1), (64, 300, -100), (64, 0, 16), (64, -1, 16), (64, 0, 0), (64, 1, -1), (2, 16, 16), (0, 16, 16), (-5, 16, 16)]:
        assert call(Sc, Ni, Sb) == L.NL_ERR_BAD_ARG, (Sc, Ni, Sb)
    for Sc, Ni, Sb in [(64, 193, 64), (64, 1, 256), (64, 257, 0), (65, 16, 16), (64, 2 ** 31 - 1, 2 ** 31 - 1)]:
        assert call(Sc, Ni, Sb) == L.NL_ERR_UNSUPPORTED, (Sc, Ni, Sb)
    assert call(64, 16, -1, R=0) == L.NL_OK, "an empty batch reads nothing"
    assert lib.nl_sample_pdf(p, p, 64, p, 16, None, 16, 4, o, None) == L.NL_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "nothing was launched"
    sc = hc.coarse_scene("hier", 3, 5, 13, False)
    r = _renderer(sc, sc["weights"])
    cam, pix, zc = _cam(sc), _dev(sc["pix"]), _dev(sc["zc"])
    w = torch.full((5, 13), float("nan"), device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    cw = lambda Sc, nbytes: lib.nl_coarse_weights(ct.byref(r.cfg), r.packed.data_ptr(), r._frame, cam.data_ptr(), pix.data_ptr(), zc.data_ptr(), 5, Sc,
                                                  w.data_ptr(), None, ws.data_ptr(), nbytes, None)
    assert [cw(2, 1), cw(0, 1), cw(-1, 1)] == [L.NL_ERR_BAD_ARG] * 3
    assert cw(65, 1) == L.NL_ERR_UNSUPPORTED
    assert cw(13, 1) == L.NL_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(w).all())


# ----------------------------------------------------------------------------- nl_coarse_weights
def _renderer(sc, weights, precision="fp32"):
    from nerf_loc_amd.renderer import HipRenderer
    cfg, fr = sc["cfg"], sc["frame"]
    r = HipRenderer(cfg.W, cfg.C, cfg.S_total, precision)
    r.load_weights({k: torch.from_numpy(v) for k, v in weights.items()})
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, fr["support_fine"])
    return r


def _cam(sc):
    """HOST 12 + 9 floats, formed like HipRenderer.hierarchical_depths forms them"""
    Kc, Pc = torch.from_numpy(sc["K"]).float(), torch.from_numpy(sc["pose"]).float()
    return torch.cat([Pc[None].inverse()[0, :3].reshape(-1), torch.inverse(Kc).reshape(-1)]).contiguous()


def _coarse(r, sc, want_depth=True):
    """nl_coarse_weights -> (weights (R, Sc), depth_coarse (R,) or None) numpy; outputs start as NaN."""
    L, lib = _L()
    R, Sc = sc["zc"].shape
    cam, pix, zc = _cam(sc), _dev(sc["pix"]), _dev(sc["zc"])
    w = torch.full((R, Sc), float("nan"), device=DEV)
    dc = torch.full((R,), float("nan"), device=DEV) if want_depth else None
    ws = L.workspace(lib.nl_coarse_weights_workspace_bytes(r.V, R, Sc), DEV, "nl_coarse_weights")
    L.check(lib.nl_coarse_weights(ct.byref(r.cfg), r.packed.data_ptr(), r._frame, cam.data_ptr(), pix.data_ptr(), zc.data_ptr(), R, Sc, w.data_ptr(), L.ptr(dc),
                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "nl_coarse_weights")
    torch.cuda.synchronize()
    return w.cpu().numpy(), None if dc is None else dc.cpu().numpy()


@pytest.mark.parametrize("name,V,shape,jitter,off_block", hc.COARSE_SCENES)
def test_coarse_weights_match_fp64(name, V, shape, jitter, off_block):
    """weights and depth_coarse of every mode against diff_render.coarse_weights_diff in double, with the decoders as synthesised and sharpened (opaque rays);
    bar = max(2e-5, 3 x the fp32 eager restatement's own deviation from fp64 on that scene), relative to the largest weight / depth.  Rays that no view sees
    (asserted from the fp64 mask) must carry the ground state's weights, to the same bar relative to the largest of THOSE; a NULL depth_coarse and a second
    call leave the bits of `weights` alone."""
    R, Sc = shape
    sc = hc.coarse_scene(name, V, R, Sc, jitter, off_block=off_block)
    px, py, dep, mask = hr.coarse_projection64(sc["frame"], sc["pix"], sc["K"], sc["pose"], sc["zc"])
    margin, dmin = hr.border_margin(sc["frame"], px, py, dep)
    assert margin > 1e-3 and dmin > 1e-3, "no sample at a mask edge"
    off = sc["off"]
    assert int(off.sum()) == off_block and not mask[:, off].any()
    fails = []
    for setting, weights in (("synthesised", sc["weights"]), ("sharpened", hc.sharpened(sc["weights"]))):
        w64 = hc.coarse_weights_ref(sc, weights, torch.float64)
        w32 = hc.coarse_weights_ref(sc, weights, torch.float32)
        d64, d32 = (w64 * sc["zc"]).sum(1), (w32 * sc["zc"]).sum(1)
        dev = max(rel_err(w32, w64), rel_err(d32, d64))
        bar = max(2e-5, 3 * dev)
        ground = hr.ground_weights(Sc)
        if off_block:
            assert np.abs(w64[off] - ground).max() < 1e-12
        r = _renderer(sc, weights)
        print(f"\n  {name} V={V} R={R} Sc={Sc} {'per-ray rows' if jitter else 'shared row'} unseen rays {off_block} {setting}: largest weight {w64.max():.4f}, "
              f"largest ray sum {w64.sum(1).max():.4f}, fp32 reference vs fp64 {dev:.1e}, bar {bar:.1e}")
        for mode in MODES:
            r.set_precision(mode)
            w, dc = _coarse(r, sc)
            ew, ed = rel_err(w, w64), rel_err(dc, d64)
            eo = float(np.abs(w[off] - ground).max() / ground.max()) if off_block else 0.0
            print(f"    {mode:7s} weights {ew:.1e}  depth_coarse {ed:.1e}" + (f"  unseen rays vs ground state {eo:.1e}" if off_block else ""))
            if not (np.isfinite(w).all() and np.isfinite(dc).all() and ew < bar and ed < bar and eo < bar):
                fails.append((setting, mode, ew, ed, eo, bar))
            w_null, _ = _coarse(r, sc, want_depth=False)
            w_again, dc_again = _coarse(r, sc)
            if not (np.array_equal(w.view(np.uint32), w_null.view(np.uint32)) and np.array_equal(w.view(np.uint32), w_again.view(np.uint32))
                    and np.array_equal(dc.view(np.uint32), dc_again.view(np.uint32))):
                fails.append((setting, mode, "bits differ between calls / with depth_coarse == NULL"))
    assert not fails, fails


# ----------------------------------------------------------------------------- the chain on the sharpened scene
@pytest.mark.parametrize("Ni", hc.CHAIN_NI)
def test_chain_on_opaque_rays_matches_fp64_resampling_of_the_kernels_own_weights(Ni):
    """HipRenderer.hierarchical_depths on the sharpened `hier` scene: the resampled depths against sample_pdf64 fed the KERNEL's coarse weights, per sample
    within hier_ref.tolerance.  The seeded draws leave no sample ill-conditioned (asserted here on the kernel's weights; chosen on the CPU on the
    reference's), and some ray has collapsed bins — the branch the thin scenes of the other tests never reach."""
    sc = hc.chain_case()
    R = len(sc["pix"])
    u = hc.chain_u(Ni, R)
    cfg = sc["cfg"]
    fails = []
    for mode in ("fp32", "bf16x3"):
        r = _renderer(sc, sc["weights"], mode)
        z, dc, wc = r.hierarchical_depths(sc["pix"], sc["K"], sc["pose"], np.full((R, 1), cfg.far + 1.0, np.float32), u, n_coarse=64)
        torch.cuda.synchronize()
        z, wc = z.cpu().numpy(), wc.cpu().numpy()
        bins = hr.mid_points32(sc["zc"])
        ref = hr.sample_pdf64(bins, wc[:, 1:-1], u)
        collapsed, _ = hr.bin_classes(ref)
        assert hr.conditioned(ref, u).all(), (mode, np.argwhere(~hr.conditioned(ref, u)).tolist())
        assert (collapsed.sum(1) > 0).any(), "a ray with collapsed bins"
        tol = hr.tolerance(ref, bins, u)
        err = np.abs(z[:, :Ni] - ref["z"])
        print(f"\n  chain Ni {Ni} {mode}: rays with collapsed bins {int((collapsed.sum(1) > 0).sum())} (most: {int(collapsed.sum(1).max())} of 62), largest ray sum "
              f"{wc.sum(1).max():.4f}, worst error / tolerance {float((err / tol).max()):.3f}, largest error {err.max() / (cfg.far - cfg.near):.1e} of the range")
        if not (np.isfinite(z).all() and (z[:, Ni] == np.float32(cfg.far + 1.0)).all() and (err <= tol).all()):
            fails.append((mode, float((err / tol).max())))
    assert not fails, fails
