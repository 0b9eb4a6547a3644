"""Seeded recipes for the stage tests of hierarchical sampling (tests/test_hier_cpu.py, tests/test_gpu_hier.py).  numpy RNG only.

Resampling (nl_sample_pdf): per ray one of WEIGHT_ROWS over one of DEPTH_ROWS, and uniforms u sorted ascending: 0.0, the mid-points of collapsed bins
below the peak, 1 - 2^-24 where the last bin is not collapsed, the rest random.  A draw that tests/hier_ref.py `conditioned` rejects is redrawn (random) or
left out (special), so every sample of every recipe is well-conditioned — tests/test_hier_cpu.py asserts it; no test excludes anything afterwards.

Coarse weights (nl_coarse_weights): the `hier` and `offview` recipes of tests/golden_cases.py shrunk to a few rays, with V in {1, 3, 16}, shared or per-ray
jittered depth rows, the decoders as synthesised or sharpened (opaque rays), and a block of rays that no view sees."""
from __future__ import annotations

import zlib

import numpy as np

from tests import hier_ref as hr

F32 = np.float32
NEAR, FAR = 2.0, 6.0
WEIGHT_ROWS = ("zeros", "onehot1", "onehot_half", "two_ends", "opaque", "thin", "only_dropped_ends")
DEPTH_ROWS = ("linear", "lindisp", "jitter")
SC = (3, 4, 5, 33, 64)
NI = (1, 7, 64, 65, 129)
RS = (1, 4, 5, 9)
# (Sc, Ni, R): every Sc x Ni; R cycles through RS so that each Sc and each Ni meets every R at least once over the list
ARITH_CASES = [(sc, ni, RS[(i + j) % 4]) for i, sc in enumerate(SC) for j, ni in enumerate(NI)]
# (Sb, Ni, Sc, R): Sb + Ni = 256 fills the sort network exactly
MERGE_CASES = [(64, 192, 64, 9), (255, 1, 33, 5), (1, 255, 5, 4), (3, 5, 3, 1), (64, 16, 4, 9)]


def weight_row(name: str, Sc: int, rng: np.random.Generator) -> np.ndarray:
    """Full-length (Sc,) fp32 row of coarse weights; the kernel drops both ends."""
    w = np.zeros(Sc)
    if name == "onehot1":
        w[Sc // 2] = 1.0
    elif name == "onehot_half":
        w[Sc // 2] = 0.5
    elif name == "two_ends":
        w[1] = 0.6
        w[Sc - 2] = 0.39
    elif name == "opaque":
        a = np.maximum(1.0 / (1.0 + np.exp(-3.0 * (np.arange(Sc) - 0.6 * Sc))), 3e-7)
        w = a * np.cumprod(np.concatenate([[1.0], 1.0 - a]))[:-1]
    elif name == "thin":
        w = rng.uniform(0.0, 0.02, Sc)
    elif name == "only_dropped_ends":
        w[0], w[-1] = 0.9, 0.1
    elif name != "zeros":
        raise KeyError(name)
    return w.astype(F32)


def depth_row(kind: str, Sc: int, rng: np.random.Generator) -> np.ndarray:
    """(Sc,) fp32 strictly increasing coarse depths in [NEAR, FAR]."""
    t = np.linspace(0.0, 1.0, Sc)
    if kind == "lindisp":
        z = 1.0 / (1.0 / NEAR * (1 - t) + 1.0 / FAR * t)
    else:
        z = NEAR * (1 - t) + FAR * t
        if kind == "jitter":
            z = z + rng.uniform(-0.4, 0.4, Sc) * (FAR - NEAR) / (Sc - 1)
            z[0], z[-1] = max(z[0], NEAR), min(z[-1], FAR)
    z = z.astype(F32)
    assert (np.diff(z) > 0).all()
    return z


def special_draws(ref1, bins1) -> list:
    """The special uniforms of one ray (ref1: hier_ref.sample_pdf64 of that ray alone), before the conditioning filter."""
    collapsed, uncertain = hr.bin_classes(ref1)
    cdf, pdf = ref1["cdf"][0], ref1["pdf"][0]
    out = [0.0]
    peak = int(np.argmax(pdf))
    below = [k for k in range(peak) if collapsed[0, k] and not uncertain[0, k]]
    for k in sorted({below[0], below[len(below) // 2], below[-1]}) if below else []:
        out.append(0.5 * (cdf[k] + cdf[k + 1]))
    if not (collapsed[0, -1] or uncertain[0, -1]):
        out.append(1.0 - 2.0 ** -24)
    return out


def draw_u(zc1, wc1, Ni: int, rng: np.random.Generator, pick: int) -> np.ndarray:
    """(Ni,) fp32 sorted uniforms for one ray: the specials that are well-conditioned (Ni = 1: one of them or a random draw, by `pick`), then random draws,
    each redrawn until `conditioned` accepts it."""
    bins = hr.mid_points32(zc1[None])
    w_in = wc1[None, 1:-1]
    good = lambda cand: hr.conditioned(hr.sample_pdf64(bins, w_in, np.asarray(cand, np.float64)[None]), np.asarray(cand, np.float64)[None])[0]
    ref1 = hr.sample_pdf64(bins, w_in, np.zeros((1, 1)))
    sp = np.asarray(special_draws(ref1, bins), F32)
    sp = sp[good(sp)]
    if Ni == 1:
        sp = sp[[(pick // 2) % len(sp)]] if (pick % 2 and len(sp)) else sp[:0]
    sp = sp[:Ni]
    u = np.concatenate([sp, rng.random(Ni - len(sp), dtype=F32)]).astype(F32)
    for _ in range(200):
        bad = ~good(u)
        if not bad.any():
            return np.sort(u)
        assert not bad[:len(sp)].any()
        u[bad] = rng.random(int(bad.sum()), dtype=F32)
    raise RuntimeError("no well-conditioned draw found")


def resample_case(Sc: int, Ni: int, R: int) -> dict:
    """-> dict(zc (R, Sc), wc (R, Sc), u (R, Ni) sorted, rows, depths: the recipe names per ray), fp32.  Ray r of a case takes weight row (k0 + r) mod 7 and
    depth row (k0 + r) mod 3, k0 fixed by (Sc, Ni, R): a case of 9 rays holds every weight row, the case list every (row, depth row, Sc) combination."""
    rng = np.random.default_rng(zlib.crc32(f"hier-resample {Sc} {Ni} {R}".encode()))
    k0 = zlib.crc32(f"hier-rows {Sc} {Ni} {R}".encode()) % 21
    rows = [WEIGHT_ROWS[(k0 + r) % 7] for r in range(R)]
    depths = [DEPTH_ROWS[(k0 + r) % 3] for r in range(R)]
    zc = np.stack([depth_row(d, Sc, rng) for d in depths])
    wc = np.stack([weight_row(n, Sc, rng) for n in rows])
    u = np.stack([draw_u(zc[r], wc[r], Ni, rng, k0 + r) for r in range(R)])
    return {"Sc": Sc, "Ni": Ni, "R": R, "zc": zc, "wc": wc, "u": u, "rows": rows, "depths": depths}


def reference(case) -> dict:
    """hier_ref.sample_pdf64 of a case plus its bins, the conditioning mask and the tolerance, each (R, Ni)."""
    bins = hr.mid_points32(case["zc"])
    ref = hr.sample_pdf64(bins, case["wc"][:, 1:-1], case["u"])
    ref.update(bins=bins, conditioned=hr.conditioned(ref, case["u"]), tolerance=hr.tolerance(ref, bins, case["u"]))
    return ref


def above_far(R: int) -> np.ndarray:
    """z_base (R, 1) beyond every depth row: with Sb = 1 it sorts last, and position i of the output is sample i (sorted u, monotone inverse CDF)."""
    return np.full((R, 1), FAR + 1.0, F32)


def base_rows(case, Sb: int) -> np.ndarray:
    """z_base (R, Sb) fp32 for the merge test, unsorted: depths spread over [NEAR, FAR] (they interleave with the resampled ones), byte-copies of bin
    mid-points (what a collapsed bin returns exactly), duplicates, one value below NEAR and one above FAR."""
    rng = np.random.default_rng(zlib.crc32(f"hier-base {case['Sc']} {case['Ni']} {case['R']} {Sb}".encode()))
    R = case["R"]
    bins = hr.mid_points32(case["zc"])
    zb = rng.uniform(NEAR, FAR, (R, Sb)).astype(F32)
    for r in range(R):
        plant = [F32(NEAR - 0.5), bins[r, bins.shape[1] // 2], F32(FAR + 0.5), bins[r, bins.shape[1] // 2], bins[r, 0], bins[r, -1]]
        if Sb == 1:
            plant = [plant[r % 3]]
        pos = rng.permutation(Sb)[:len(plant)]
        zb[r, pos] = plant[:len(pos)]
        if Sb >= 16:
            zb[r, rng.permutation(Sb)[:4]] = zb[r, rng.integers(0, Sb)]      # five equal keys
    return zb


def zeros_closed_form(case) -> np.ndarray:
    """(R, Ni) double: all-zero weights make the pdf uniform, so the inverse CDF is the piecewise-linear interpolation of the bins over u * nb."""
    bins = hr.mid_points32(case["zc"]).astype(np.float64)
    nb = bins.shape[1] - 1
    return np.stack([np.interp(u.astype(np.float64) * nb, np.arange(nb + 1), b) for u, b in zip(case["u"], bins)])


def arith_failures(case, ref, z_out) -> list:
    """What the arithmetic test asserts about z_out (R, 1 + Ni) = the stage's answer to (case, z_base = above_far): the samples in output positions 0 .. Ni - 1
    within `tolerance` of the fp64 restatement (and, on `zeros` rows, of the closed form), the base depth last, nothing left unwritten.  -> list of failures."""
    z_out = np.asarray(z_out)
    Ni = case["Ni"]
    fails = []
    if z_out.shape != (case["R"], Ni + 1) or not np.isfinite(z_out).all():
        return [("shape / not finite", z_out.shape, int((~np.isfinite(z_out)).sum()))]
    if not np.array_equal(z_out[:, Ni:], above_far(case["R"])):
        fails.append(("the base depth is not last", z_out[:, Ni:].ravel().tolist()))
    err = np.abs(z_out[:, :Ni].astype(np.float64) - ref["z"])
    bad = err > ref["tolerance"]
    for r, i in zip(*np.nonzero(bad)):
        fails.append((case["rows"][r], case["depths"][r], f"ray {r} sample {i} u {case['u'][r, i]!r} err {err[r, i]:.3e} tol {ref['tolerance'][r, i]:.3e}"))
    closed = zeros_closed_form(case)
    for r, name in enumerate(case["rows"]):
        if name == "zeros" and (np.abs(z_out[r, :Ni] - closed[r]) > ref["tolerance"][r]).any():
            fails.append(("zeros: closed form", r))
    return fails


def merge_failures(zb, zf, z_out) -> list:
    """The merge is exact: z_out must be np.sort(concat(z_base, zf)) bit for bit, zf being the stage's own samples."""
    want = np.sort(np.concatenate([zb, zf], 1), 1)
    z_out = np.asarray(z_out)
    if z_out.shape != want.shape:
        return [("shape", z_out.shape)]
    diff = want.view(np.uint32) != z_out.view(np.uint32)
    return [(f"ray {r} position {i}: {z_out[r, i]!r} for {want[r, i]!r}") for r, i in zip(*np.nonzero(diff))]


# ----------------------------------------------------------------------------- coarse weights
SHARPEN = {"multiview_aggregator.dist_decoder.var_decoder.4.bias": 400.0, "multiview_aggregator.dist_decoder.vis_decoder.4.bias": 9.0}
# (R, Sc): fewest rows; one past two 32-row tiles of the MFMA kernel; odd sizes; Sc = 64
COARSE_SHAPES = [(1, 3), (5, 13), (7, 33), (16, 64)]
COARSE_VIEWS = (1, 3, 16)
OFF_PIX = (6000.0, -4500.0)   # a pixel whose ray leaves every support view's image after the first millimetre
# (recipe, V, (R, Sc), per-ray jittered depth rows, how many of the R rays are unseen ones, placed after the first ray).  `hier`: every shape with every V; `offview` (a view
# that looks backwards, one far to the side, one inside the volume): every shape.  Two or three unseen rays are 99 / 128 consecutive rows: at least two whole
# 32-row tiles of the MFMA kernel that no view sees, between tiles that are seen.
COARSE_SCENES = [("hier", v, s, bool((i + j) % 2), {(1, 1): 1, (2, 0): 3, (3, 2): 2}.get((i, j), 0))
                 for i, s in enumerate(COARSE_SHAPES) for j, v in enumerate(COARSE_VIEWS)]
COARSE_SCENES += [("offview", 3, (1, 3), True, 0), ("offview", 16, (5, 13), False, 0), ("offview", 1, (7, 33), True, 3), ("offview", 3, (16, 64), False, 0)]
# seeds other than the golden recipe's own, where that one puts a sample within 1e-3 px of a view's border (tests/test_hier_cpu.py checks every scene)
COARSE_SEEDS = {('hier', 16, 16, 64, True): 107, ('offview', 3, 16, 64, False): 101}


def sharpened(weights: dict) -> dict:
    """The decoders that make surfaces: +400 on the variance decoder's last bias (a step-like cdf), +9 on the visibility decoder's (visibility ~ 1)."""
    out = dict(weights)
    for k, add in SHARPEN.items():
        out[k] = (weights[k] + F32(add)).astype(F32)
    return out


def coarse_scene(name: str, V: int, R: int, Sc: int, jitter: bool, seed: int | None = None, off_block: int = 0) -> dict:
    """-> dict(cfg, frame, weights, pix (R, 2), zc (R, Sc), K, pose, off (R,) bool): golden recipe `name` ('hier' or 'offview') with V views and R rays;
    `jitter`: every ray has its own depth row; off_block > 0: that many of the R rays, consecutive after the first one, go through OFF_PIX."""
    from nerf_loc_amd.synth import make_frame, make_rays, make_weights
    from tests.golden_cases import CASES
    cfg = CASES[name][0]
    seed = COARSE_SEEDS.get((name, V, R, Sc, jitter), cfg.seed) if seed is None else seed
    cfg = cfg.replace(name=f"{name}_coarse", V=V, R=R - off_block, seed=seed)
    frame = make_frame(cfg)
    if name == "offview":   # tests/golden_cases.py build_case, for the views that exist
        poses = frame["topk_poses"]
        if V > 1:
            poses[1, :3, :3] = poses[1, :3, :3] @ np.diag([-1.0, 1.0, -1.0]).astype(F32)
        if V > 2:
            poses[2, :3, 3] += np.array([30.0, 0, 0], F32)
        if V > 3:
            poses[3, :3, 3] += np.array([0, 0, 2.0], F32)
    rays = make_rays(cfg, frame)
    pix = rays["pixel_coordinates"]
    off = np.zeros(R - off_block, bool)
    if off_block:
        pix = np.concatenate([pix[:1], np.tile(np.asarray(OFF_PIX, F32), (off_block, 1)), pix[1:]]).astype(F32)
        off = np.concatenate([off[:1], np.ones(off_block, bool), off[1:]])
    rng = np.random.default_rng(cfg.seed + 4000 + Sc)
    t = np.linspace(0.0, 1.0, Sc)
    zc = np.tile(cfg.near * (1 - t) + cfg.far * t, (len(pix), 1))
    if jitter:
        zc = zc + rng.uniform(-0.4, 0.4, zc.shape) * (cfg.far - cfg.near) / (Sc - 1)
        zc[:, 0], zc[:, -1] = np.maximum(zc[:, 0], cfg.near), np.minimum(zc[:, -1], cfg.far)
    zc = zc.astype(F32)
    assert (np.diff(zc, axis=1) > 0).all()
    return {"cfg": cfg, "frame": frame, "weights": make_weights(cfg), "pix": np.ascontiguousarray(pix), "zc": zc, "K": frame["K"], "pose": frame["pose"], "off": off}


def coarse_weights_ref(scene, weights, dtype):
    """nerf_loc_amd.diff_render.coarse_weights_diff on the CPU in `dtype` (torch.float64: the reference; torch.float32: its own fp32 deviation) -> (R, Sc) numpy."""
    import torch
    from nerf_loc_amd import diff_render as dr
    cfg, frame = scene["cfg"], scene["frame"]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    p = {k: t(v) for k, v in weights.items() if "dist_decoder" in k}
    fr = {k: t(frame[k]) for k in ("topk_Ks", "topk_poses", "topk_images", "vis_featmaps")}
    fr.update(near=float(cfg.near), far=float(cfg.far))
    with torch.no_grad():
        return dr.coarse_weights_diff(p, fr, t(scene["pix"]), t(scene["K"]), t(scene["pose"]), t(scene["zc"])).double().numpy()


# ----------------------------------------------------------------------------- the chain: coarse weights -> resampling on the sharpened `hier` scene
CHAIN_NI = (16, 128)
CHAIN_SEEDS = {16: 0, 128: 1}   # chosen on the CPU (tests/test_hier_cpu.py): no draw falls where the resampling is ill-conditioned


# rays of make_rays(R = 512) on the `hier` frame: the recipe's own 16 rays have no collapsed bin (the decoders' alpha floor log(1e-5) keeps every weight
# above 1e-5 T, so a bin collapses only behind a surface that leaves T < 3e-4 and not on the last sample: 5 rays of 512), so the five that do are taken
# in, spread over the four-ray workgroups
CHAIN_RAYS = (0, 51, 1, 2, 145, 3, 4, 5, 287, 6, 7, 341, 8, 9, 431, 10)


def chain_case() -> dict:
    """Golden recipe `hier` (frame, 3 views, sharpened decoders, 64 coarse samples on the shared linear row) with the 16 rays CHAIN_RAYS."""
    from tests.golden_cases import CASES
    cfg = CASES["hier"][0]
    sc = coarse_scene("hier", cfg.V, 512, 64, False, seed=cfg.seed)
    import torch
    from oracle.render_oracle import sample_depths
    sel = np.asarray(CHAIN_RAYS)
    zc = sample_depths(64, torch.tensor(cfg.near), torch.tensor(cfg.far)).expand(len(sel), 64).contiguous().numpy()   # the row hierarchical_depths forms
    sc.update(pix=np.ascontiguousarray(sc["pix"][sel]), zc=zc, off=sc["off"][sel], weights=sharpened(sc["weights"]))
    return sc


def chain_u(Ni: int, R: int, seed: int | None = None) -> np.ndarray:
    """(R, Ni) fp32 uniforms, sorted per ray."""
    rng = np.random.default_rng(9000 + 100 * Ni + (CHAIN_SEEDS[Ni] if seed is None else seed))
    return np.sort(rng.random((R, Ni), dtype=F32), 1)
