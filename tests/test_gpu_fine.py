"""GPU tests of the fine matcher (csrc/fine.hip through nl_fine_windows / nl_fine_match and nerf_loc_amd.fine_matching): window rows, coordinates, heat-maps
and std against the reference's goldens, both input layouts, batch invariance, the module path and its weight cache."""
import os

import numpy as np
import pytest
import torch

from tests import fine_cases as fc
from tests import fine_ref as fr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")   # the modes held to the bars (bf16: throughput mode, not held)
BAR = 1e-4
# std = sum of sqrt(max(var, 1e-10)) with var = sum(g^2 h) - coords^2, a difference that cancels for nearly one-hot heat-maps: a match's bound is
# BAR + STD_K * d_m, d_m = |std_ref(fp32) - std_ref(fp64)| (tests/fine_ref.py: std_sensitivity).  Measured on the MI355X on the first run, over the `peaked` case
# and the matches with d_m > 1e-5 (19 of 96; below that the plain bar decides): worst |error| / d_m = 3.61, in fp32 and bf16x3 alike (the same match: the
# reference's fp32 variance falls under the clamp there).  STD_K = twice that, rounded up.  DESIGN.md §5.30.
STD_K = 8.0
DEV = "cuda:0"

_CACHE = {}


def _case(name):
    """Recipe, golden and the fp32 / fp64 sensitivity of a case: computed once per session, never modified."""
    if name not in _CACHE:
        c, g = fc.make_case(name), fc.load_golden(GOLDEN, name)
        d = fr.std_sensitivity(c["feat_f0"], g["feat_f1"], c["mlp"], c["mkps2d_c"])
        _CACHE[name] = (c, g, d)
    return _CACHE[name]


def _modules(c, mode):
    from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess
    pre = FinePreprocess(fc.preprocess_config(c["case"]), precision=mode)
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    fm = FineMatching(fc.matching_config(c["case"]), precision=mode)
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
    return pre.to(DEV).eval(), fm.to(DEV).eval()


def _feat(c, nhwc):
    f = torch.from_numpy(c["feat_f"]).to(DEV)
    if nhwc:   # what Matcher passes: a permuted view of an NHWC tensor
        f = f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not f.is_contiguous() and f.permute(0, 2, 3, 1).is_contiguous()
    return f


def _windows(pre, c, nhwc=True, sel=None):
    b, j = c["b_ids"], c["j_ids"]
    if sel is not None:
        b, j = b[sel], j[sel]
    out = pre.windows(_feat(c, nhwc), torch.from_numpy(b).to(DEV), torch.from_numpy(j).to(DEV), c["case"].s)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _match(fm, f0, f1, kc, heat=True):
    e, k, h = fm.match(torch.from_numpy(np.ascontiguousarray(f0)).to(DEV), torch.from_numpy(np.ascontiguousarray(f1)).to(DEV),
                       torch.from_numpy(np.ascontiguousarray(kc)).to(DEV), want_heatmap=heat)
    torch.cuda.synchronize()
    return e.cpu().numpy(), k.cpu().numpy(), (h.cpu().numpy() if heat else None)


def _check_match(tag, e, k, h, g, d):
    """The three parts of the comparison with the golden; returns the worst |std error| / d_m over the matches with d_m > 1e-5 (0 if none)."""
    ec = np.abs(e[:, :2].astype(np.float64) - g["expec_f"][:, :2]).max()
    ek = np.abs(k.astype(np.float64) - g["mkps2d_f"]).max()
    es = np.abs(e[:, 2].astype(np.float64) - g["expec_f"][:, 2])
    big = d > 1e-5
    ratio = float((es[big] / d[big]).max()) if big.any() else 0.0
    msg = f"fine match {tag}: coords {ec:.2e} mkps2d_f {ek:.2e} std {es.max():.2e} (worst |error| / d_m where d_m > 1e-5: {ratio:.2f}, {int(big.sum())} matches)"
    if h is not None:
        eh = np.abs(h.astype(np.float64) - g["heatmap"]).sum(axis=1).max()
        msg += f" heat-map L1 {eh:.2e}"
    print(msg)
    bad = [what for what, ok in (("coords", ec <= BAR), ("mkps2d_f", ek <= BAR), ("heat-map", h is None or eh <= BAR), ("std", bool(np.all(es <= BAR + STD_K * d)))) if not ok]
    assert not bad, f"{msg}: over the bar: {bad}"
    return ratio


# ------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", fc.GOLDEN_CASES)
def test_windows_against_the_reference_goldens(name, mode):
    c, g, _ = _case(name)
    pre, _ = _modules(c, mode)
    rows = _windows(pre, c)
    ref = g["feat_f1"]
    scale = np.abs(ref).max()
    err = np.abs(rows.astype(np.float64) - ref).max()
    pad = fr.padded_cells(c["case"].Hf, c["case"].Wf, c["j_ids"], c["case"].s)
    epad = np.abs(rows[pad].astype(np.float64) - c["proj"]["proj.bias"]).max() if pad.any() else 0.0
    print(f"fine windows {name} {mode}: max abs error {err:.3e} of {scale:.3f} ({err / scale:.2e}); padded cells vs bias {epad:.2e} ({int(pad.sum())} cells)")
    assert rows.shape == ref.shape
    assert err <= BAR * scale and epad <= BAR * scale
    if name == "borders":
        assert pad.sum(axis=1).max() == 33
    # the plain NCHW layout (one NHWC copy inside) gives the same bits
    assert np.array_equal(_windows(pre, c, nhwc=False), rows)
    assert pre.pack_count == 1


# ------------------------------------------------------------------------------------------ match
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", fc.GOLDEN_CASES)
def test_match_against_the_reference_goldens(name, mode):
    """coords and mkps2d_f: abs <= 1e-4; heat-map: L1 per match <= 1e-4; std: 1e-4 + STD_K * d_m.

    Measured on the MI355X, worst over the cases: fp32 coords 3.2e-6, mkps2d_f 9.5e-6, heat-map 5.2e-6; bf16x3 5.2e-6, 1.5e-5, 1.3e-5 (all three in `peaked`).
    bf16x3 multiplies as three-term split-FP16 in this kernel: as split-bf16 the `peaked` case (softmax arguments of +-25) reached 1.79e-4 on the heat-map and
    2.75e-4 on mkps2d_f.  DESIGN.md §5.30."""
    c, g, d = _case(name)
    _, fm = _modules(c, mode)
    e, k, h = _match(fm, c["feat_f0"], g["feat_f1"], c["mkps2d_c"])
    _check_match(f"{name} {mode}", e, k, h, g, d)
    e2, k2, h2 = _match(fm, c["feat_f0"], g["feat_f1"], c["mkps2d_c"], heat=False)     # heatmap = NULL: the same bits
    assert h2 is None and np.array_equal(e2, e) and np.array_equal(k2, k)
    if name == "flat":
        assert np.abs(e[:, :2]).max() <= 1e-6 and np.abs(e[:, 2] - 4.0 / 3.0).max() <= 1e-6 and np.abs(h - 1.0 / 49.0).max() <= 1e-7


# ------------------------------------------------------------------------------------------ invariance
@pytest.mark.parametrize("mode", MODES)
def test_outputs_do_not_depend_on_the_batch(mode):
    """A match's outputs are the same bits alone, in the full batch and at another position (c192: more than one 64-row tile group, M a multiple of nothing)."""
    c, g, _ = _case("c192")
    pre, fm = _modules(c, mode)
    M = len(c["j_ids"])
    rows = _windows(pre, c)
    e, k, h = _match(fm, c["feat_f0"], g["feat_f1"], c["mkps2d_c"])
    perm = np.random.default_rng(5).permutation(M)
    rows_p = _windows(pre, c, sel=perm)
    assert np.array_equal(rows_p, rows[perm])
    ep, kp, hp = _match(fm, c["feat_f0"][perm], g["feat_f1"][perm], c["mkps2d_c"][perm])
    assert np.array_equal(ep, e[perm]) and np.array_equal(kp, k[perm]) and np.array_equal(hp, h[perm])
    for m in (0, 3, 33, M - 1):
        sel = np.array([m])
        assert np.array_equal(_windows(pre, c, sel=sel), rows[sel]), m
        e1, k1, h1 = _match(fm, c["feat_f0"][sel], g["feat_f1"][sel], c["mkps2d_c"][sel])
        assert np.array_equal(e1, e[sel]) and np.array_equal(k1, k[sel]) and np.array_equal(h1, h[sel]), m
    for a, b in ((1, 6), (30, 67)):   # slices that start inside a workgroup's four matches
        sel = np.arange(a, b)
        assert np.array_equal(_windows(pre, c, sel=sel), rows[sel])
        e1, _, h1 = _match(fm, c["feat_f0"][sel], g["feat_f1"][sel], c["mkps2d_c"][sel])
        assert np.array_equal(e1, e[sel]) and np.array_equal(h1, h[sel])


# ------------------------------------------------------------------------------------------ through the modules
@pytest.mark.parametrize("name", ("small", "c192", "repeat"))
def test_module_chain_equals_the_reference_chain_and_caches_its_weights(name):
    c, g, d = _case(name)
    pre, fm = _modules(c, "bf16x3")
    data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": torch.from_numpy(c["b_ids"]).to(DEV),
            "j_ids": torch.from_numpy(c["j_ids"]).to(DEV), "mkps2d_c": torch.from_numpy(c["mkps2d_c"]).to(DEV), "kept": 1}
    f0 = torch.from_numpy(c["feat_f0"]).to(DEV)
    with torch.no_grad():
        f1 = pre(_feat(c, True), None, data)            # (identity in place of the transformer)
        out = fm(f0, f1, data)
    torch.cuda.synchronize()
    assert out is data and data["kept"] == 1 and tuple(f1.shape) == g["feat_f1"].shape
    assert data["expec_f"].dtype == torch.float32 and data["expec_f"].device == f0.device and tuple(data["mkps2d_f"].shape) == (len(c["j_ids"]), 2)
    _check_match(f"module chain {name}", data["expec_f"].cpu().numpy(), data["mkps2d_f"].cpu().numpy(), None, g, d)
    assert pre.pack_count == 1 and fm.pack_count == 1
    with torch.no_grad():
        pre(_feat(c, False), None, data)
        fm(f0, f1, data)
    assert pre.pack_count == 1 and fm.pack_count == 1                                   # cached
    with torch.no_grad():
        pre.proj.bias.add_(1.0)                                                         # in place: _version changes
        fm.mlps[4].bias.add_(1.0)
        f1b = pre(_feat(c, True), None, data)
        fm(f0, f1, data)
    torch.cuda.synchronize()
    assert pre.pack_count == 2 and fm.pack_count == 2
    assert np.abs(f1b.cpu().numpy() - (g["feat_f1"] + 1.0)).max() <= BAR * (np.abs(g["feat_f1"]).max() + 1.0)
    assert np.abs(data["expec_f"][:, :2].cpu().numpy() - g["expec_f"][:, :2]).max() <= BAR     # a constant added to every logit leaves the softmax alone
    # ids outside the window grid fail the host-side check
    bad = {**data, "j_ids": data["j_ids"].clone()}
    Ly, Lx = fc.grid_shape(c["case"].Hf, c["case"].Wf, c["case"].s)
    bad["j_ids"][0] = Ly * Lx
    with pytest.raises(RuntimeError, match="invalid argument|-1"):
        pre(_feat(c, True), None, bad)
    empty = {**data, "j_ids": data["j_ids"][:0], "b_ids": data["b_ids"][:0], "mkps2d_c": data["mkps2d_c"][:0]}
    with torch.no_grad():
        f1e = pre(_feat(c, True), None, empty)
        assert tuple(f1e.shape) == (0, 49, c["case"].Cout) and fm(f0[:0], f1e, empty) is None and tuple(empty["expec_f"].shape) == (0, 3)


def test_bf16_mode_runs_and_is_finite():
    c, g, _ = _case("c192")
    pre, fm = _modules(c, "bf16")
    rows = _windows(pre, c)
    e, k, h = _match(fm, c["feat_f0"], rows, c["mkps2d_c"])
    assert np.isfinite(rows).all() and np.isfinite(e).all() and np.isfinite(k).all() and np.isfinite(h).all()
    assert np.abs(h.sum(axis=1) - 1.0).max() <= 1e-5
    print(f"fine bf16 c192: rows {np.abs(rows - g['feat_f1']).max() / np.abs(g['feat_f1']).max():.2e} coords {np.abs(e[:, :2] - g['expec_f'][:, :2]).max():.2e}")
