"""fp64 numpy restatement of the hierarchical resampling stage (nl_sample_pdf, csrc/hier.hip: sample_pdf_kernel), the rule that says which of its
samples an fp32 evaluation can be compared on, the tolerance such a sample is held to, and an fp32 emulation of the kernel's own arithmetic.

Inverse-CDF sampling of a piecewise-constant pdf (conditional_nerf/utils.py:73-112, oracle.render_oracle.sample_pdf) is a discontinuous function in two places:
  1. `den < eps -> 1`: a bin whose cdf step is below eps = 1e-5 is "collapsed": every u inside it maps to (nearly) its lower edge b_lo.  At its upper knot the
     result jumps from b_lo to b_hi, a whole bin.
  2. the classification `den < eps` itself: behind an opaque sample every bin's pdf is 1e-5 / tot ~ 0.9994e-5, the cdf is ~1 there and its fp32 spacing 6e-8,
     so `den` lands on one side of eps or the other by rounding.
Two correct fp32 evaluations differ by a bin at such a sample.  `conditioned` marks them; tests/hier_cases.py places no sample there and
tests/test_hier_cpu.py asserts that (a condition on the inputs, checked without a GPU); every other sample is held to `tolerance`.

Error model (fp32, unit roundoff U = 2^-24, nb = Sc - 2 bins):
  knot     an fp32 cdf knot c is off by at most E(c) = gamma c + U, gamma = (2 nb + 4) U: the sequential sum of nb positive terms (nb U c), one division per
           term (U c), one rounded total whatever its summation order (nb U c), the rounding of w + eps (U c), slack for second-order terms (2 U c), + U absolute.
  step     the cdf step of ONE bin, den = c_hi - c_lo as fp32 forms it, is off by far less than E where c is small: c_hi = fl(c_lo + p) adds one rounding
           (<= U c_hi), the difference another (<= U den), and p = fl(fl(w + eps) / tot) carries the relative error of the total and the division
           (<= (nb + 2) U):   D(c_hi, den) = gamma den + 2 U c_hi.
A sample (bin k: c_k <= u < c_k+1; u >= c_nb: the clamp makes lo = hi = nb) is WELL-CONDITIONED iff
  (a) |den_k - eps| > 2 D(c_k+1, den_k): the class of its own bin is the same in every fp32 evaluation;
  (b) u is farther than 2 E from the upper knot of every bin that is collapsed OR whose class (a) cannot tell: the jump of 1.;
  (c) u is farther than 2 E from cdf[nb] unless the last bin is certainly not collapsed (at and beyond cdf[nb] the result is bins[nb]; a collapsed last bin
      returns bins[nb - 1] just below it).
The class of a NEIGHBOURING bin matters only through its upper knot — an fp32 evaluation can place u in a neighbour only within E of the shared knot, and
the function is continuous across a knot unless the bin below it is collapsed — so (b) carries it, for every bin and not just the neighbours.  (Holding a
neighbour's step to |den - eps| > 2 E(c_hi) regardless of u would reject every sample inside the peak of a one-hot ray: the bin behind the peak has
|den - eps| = 6e-9 at c ~ 1.  Holding the sample's own bin to E instead of D would reject every collapsed bin: |den - eps| = nb 1e-10 there, below U.)

tolerance = (b_hi - b_lo) min(1, 2 E(max(c_hi, u)) / den_used) + 8 U max|bins|: both knots of the bin move by E, u - c_lo over den_used moves by 2 E / den_used
at most and never by more than the whole bin; 8 U max|bins| covers the roundings of the closing  b_lo + t (b_hi - b_lo)  and of the fp32 mid-points themselves.
It is derived, not tuned: a well-conditioned sample beyond it is a finding about the code under test."""
from __future__ import annotations

import numpy as np

EPS = 1e-5
U24 = 2.0 ** -24
PAD = np.float32(3.4e38)   # the kernel's sort padding


def gamma(nb: int) -> float:
    return (2 * nb + 4) * U24


def knot_error(c, nb: int, unit: float = U24):
    """E(c): bound on |cdf knot formed with unit roundoff `unit` - exact knot| (fp32 unless said otherwise)."""
    return (gamma(nb) * np.asarray(c, np.float64) + U24) * (unit / U24)


def step_error(c_hi, den, nb: int):
    """D(c_hi, den): bound on |fp32 cdf step of one bin - exact step|."""
    return gamma(nb) * np.asarray(den, np.float64) + 2 * U24 * np.asarray(c_hi, np.float64)


def sample_pdf64(bins, w_inner, u):
    """oracle.render_oracle.sample_pdf in double.  bins (R, nb + 1), w_inner (R, nb) = weights[:, 1:-1], u (R, Ni)
    -> dict z (R, Ni), cdf (R, nb + 1), pdf (R, nb), lo, hi (R, Ni) int, den (R, Ni) = cdf[hi] - cdf[lo] BEFORE the `den < eps -> 1` replacement."""
    bins, w_inner, u = (np.asarray(a, np.float64) for a in (bins, w_inner, u))
    nb = w_inner.shape[1]
    w = w_inner + EPS
    pdf = w / w.sum(-1, keepdims=True)
    cdf = np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, -1)], -1)
    inds = np.stack([np.searchsorted(c, uu, side="right") for c, uu in zip(cdf, u)])
    lo, hi = np.maximum(inds - 1, 0), np.minimum(inds, nb)
    c_lo, c_hi = np.take_along_axis(cdf, lo, 1), np.take_along_axis(cdf, hi, 1)
    b_lo, b_hi = np.take_along_axis(bins, lo, 1), np.take_along_axis(bins, hi, 1)
    den = c_hi - c_lo
    used = np.where(den < EPS, 1.0, den)
    return {"z": b_lo + (u - c_lo) / used * (b_hi - b_lo), "cdf": cdf, "pdf": pdf, "lo": lo, "hi": hi, "den": den}


def bin_classes(ref):
    """-> (collapsed, uncertain), each (R, nb) bool: the bin's cdf step is below eps; rule (a) cannot tell on which side of eps an fp32 step lands."""
    cdf = ref["cdf"]
    nb = cdf.shape[1] - 1
    step = cdf[:, 1:] - cdf[:, :-1]
    return step < EPS, np.abs(step - EPS) <= 2 * step_error(cdf[:, 1:], step, nb)


def conditioned(ref, u):
    """(R, Ni) bool: the samples on which two correct fp32 evaluations agree to `tolerance` (module docstring, rules a-c)."""
    u = np.asarray(u, np.float64)
    cdf = ref["cdf"]
    nb = cdf.shape[1] - 1
    collapsed, uncertain = bin_classes(ref)
    k = np.minimum(ref["lo"], nb - 1)                                    # the sample's bin (u >= cdf[nb]: judged like the last bin, and by rule c)
    ok = ~np.take_along_axis(uncertain, k, 1)                            # (a)
    jump = collapsed | uncertain
    knots = cdf[:, 1:]
    far = np.abs(u[:, :, None] - knots[:, None, :]) > 2 * knot_error(np.maximum(knots[:, None, :], u[:, :, None]), nb)
    ok &= (far | ~jump[:, None, :]).all(-1)                              # (b)
    last = jump[:, -1][:, None]
    ok &= ~last | (np.abs(u - cdf[:, -1:]) > 2 * knot_error(np.maximum(cdf[:, -1:], u), nb))   # (c)
    return ok


def tolerance(ref, bins, u, unit: float = U24):
    """(R, Ni): the bound |fp32 sample - ref['z']| of a well-conditioned sample (module docstring).  `unit` = 2^-53 gives the same bound for two evaluations
    in double, which differ by the rounding of the total too: 1e-16 / den of a bin, 1e-11 of its width where den ~ 1e-5."""
    bins, u = np.asarray(bins, np.float64), np.asarray(u, np.float64)
    nb = bins.shape[1] - 1
    c_hi = np.take_along_axis(ref["cdf"], ref["hi"], 1)
    width = np.take_along_axis(bins, ref["hi"], 1) - np.take_along_axis(bins, ref["lo"], 1)
    used = np.where(ref["den"] < EPS, 1.0, ref["den"])
    return width * np.minimum(1.0, 2 * knot_error(np.maximum(c_hi, u), nb, unit) / used) + 8 * unit * np.abs(bins).max()


def mid_points32(zc):
    """The bins as the kernel forms them: 0.5f * (zc[i] + zc[i + 1]) in fp32."""
    zc = np.asarray(zc, np.float32)
    return (np.float32(0.5) * (zc[:, :-1] + zc[:, 1:])).astype(np.float32)


# ----------------------------------------------------------------------------- fp32 emulation of sample_pdf_kernel, with the one-line mutations the tests must catch
MUTATIONS = ("den_eps_dropped", "above_clamped_low", "cdf_inclusive", "pad_zero")


def _wave_sum32(x64):
    """a 64-lane butterfly sum in fp32 (the order of wave_sum; any order is inside the error model)"""
    t = np.asarray(x64, np.float32).copy()
    o = 32
    while o >= 1:
        t = (t + np.roll(t, -o)).astype(np.float32)
        o //= 2
    return t[0]


def sample_pdf_kernel32(zc, wc, u, zb, mutation=None):
    """sample_pdf_kernel's arithmetic, operation by operation in fp32 on the CPU: zc, wc (R, Sc), u (R, Ni), zb (R, Sb) -> z_out (R, Sb + Ni) fp32.
    `mutation` breaks one line the way a subtly wrong kernel would (tests/test_hier_cpu.py shows that the stage tests catch each)."""
    assert mutation is None or mutation in MUTATIONS
    f32 = np.float32
    zc, wc, u, zb = (np.asarray(a, f32) for a in (zc, wc, u, zb))
    R, Sc = zc.shape
    nb, Ni, Sb = Sc - 2, u.shape[1], zb.shape[1]
    bins = mid_points32(zc)
    out = np.empty((R, Sb + Ni), f32)
    eps = f32(EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(R):
            wgt = np.zeros(64, f32)
            wgt[:nb] = wc[r, 1:Sc - 1] + eps
            pdf = (wgt / _wave_sum32(wgt)).astype(f32)
            cdf = np.zeros(nb + 1, f32)
            run = f32(0)
            for i in range(nb):
                run = f32(run + pdf[i])
                cdf[i + 1] = run
            if mutation == "cdf_inclusive":
                cdf = np.concatenate([cdf[1:], cdf[-1:]])
            keys = np.full(256, f32(0) if mutation == "pad_zero" else PAD, f32)
            keys[:Sb] = zb[r]
            for i in range(Ni):
                uu = u[r, i]
                lo = int(np.searchsorted(cdf, uu, side="right"))
                below = max(lo - 1, 0)
                above = min(lo, nb - 1 if mutation == "above_clamped_low" else nb)
                c0, c1, b0, b1 = cdf[below], cdf[above], bins[r, below], bins[r, above]
                den = f32(c1 - c0)
                if den < eps and mutation != "den_eps_dropped":
                    den = f32(1)
                keys[Sb + i] = f32(b0 + f32(f32(f32(uu - c0) / den) * f32(b1 - b0)))
            out[r] = np.sort(keys)[:Sb + Ni]   # NaN (a mutation's 0 / 0) sorts last
    return out


# ----------------------------------------------------------------------------- coarse weights: fp64 projection into the support views
def coarse_projection64(frame, pix, K, pose, zc):
    """The projection of nerf_loc_amd.diff_render.coarse_weights_diff (depth_fusion.py:9-45, multiview_aggregator.py:95-120) in numpy double:
    -> px, py, depth, mask, each (V, R, Sc): pixel position and camera depth of every coarse sample in every support view, and the in-view mask."""
    d = lambda a: np.asarray(a, np.float64)
    pix, zc = d(pix), d(zc)
    H, W = frame["topk_images"].shape[-2:]
    q_w2c = np.linalg.inv(d(pose))[:3]
    rot = q_w2c[:, :3].T
    cen = -rot @ q_w2c[:, 3]
    cam = np.linalg.inv(d(K)) @ np.concatenate([pix, np.ones((pix.shape[0], 1))], 1).T
    dirs = (rot @ cam).T
    pts = cen[None, None, :] + dirs[:, None, :] * zc[..., None]
    px, py, dep = [], [], []
    for Kv, Pv in zip(d(frame["topk_Ks"]), d(frame["topk_poses"])):
        P = Kv @ np.linalg.inv(Pv)[:3]
        c = pts @ P[:, :3].T + P[:, 3]
        px.append(c[..., 0] / c[..., 2])
        py.append(c[..., 1] / c[..., 2])
        dep.append(c[..., 2])
    px, py, dep = np.stack(px), np.stack(py), np.stack(dep)
    mask = (np.abs(dep) >= 1e-4) & ~((px < -0.5) | (px >= W - 0.5) | (py < -0.5) | (py >= H - 0.5))
    return px, py, dep, mask


def border_margin(frame, px, py, dep):
    """-> (smallest distance in px of any sample to a border of a view's mask rectangle, smallest |depth|)"""
    H, W = frame["topk_images"].shape[-2:]
    m = min(float(np.abs(px + 0.5).min()), float(np.abs(px - (W - 0.5)).min()), float(np.abs(py + 0.5).min()), float(np.abs(py - (H - 0.5)).min()))
    return m, float(np.abs(dep).min())


def ground_weights(Sc: int):
    """Weights of a ray no view sees: alpha = sigmoid(-15) at every sample, composited front to back."""
    a = 1.0 / (1.0 + np.exp(15.0))
    return a * (1.0 - a) ** np.arange(Sc)


def coarse_ray64(alpha, vis, mask, ignore_nmask=False):
    """coarse_ray_kernel's reduction over the views in double: alpha, vis, mask (V, R, Sc) -> weights (R, Sc).  `ignore_nmask` is the mutation
    'a sample no view sees is not sent to the ground state' (tests/test_hier_cpu.py)."""
    a = alpha * mask + (1 - mask) * -15.0
    vs = vis * mask
    al = (a * vs).sum(0) / np.maximum(vs.sum(0), 1e-8)
    if not ignore_nmask:
        al = np.where(mask.sum(0) == 0, -15.0, al)
    s = 1.0 / (1.0 + np.exp(-al))
    T = np.cumprod(np.concatenate([np.ones_like(s[:, :1]), 1 - s], 1)[:, :-1], 1)
    return s * T
