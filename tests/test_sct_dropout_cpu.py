"""CPU-side tests of the SelfCrossTransformer's dropout (csrc/sct_drop.h as restated in tests/sct_dropout_ref.py): the generator against the published known-answer
vectors, the statistics and the independence of the masks, their invariance to how a call is cut, the goldens against the fp64 restatement, the argument checks of
the dropout entry points that need no GPU, and the CPU fall-back of hip_dropout."""
import ctypes as ct
import math
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_dropout_ref as dr
from tests import sct_train_cases as stc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("out0", "out1") + stc.INPUT_GRADS + stc.PARAM_NAMES


def test_philox_known_answers():
    """The three vectors published with the algorithm (Random123's kat_vectors: philox4x32, 10 rounds)."""
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert " ".join(f"{int(w):08x}" for w in dr.philox4x32_10(*ctr, *key)) == want


def test_threshold_and_scale():
    assert dr.threshold(0.0) == 0 and dr.threshold(0.1) == 6554 and dr.threshold(0.5) == 32768 and dr.threshold(0.9999999) == 65535
    for p in (0.1, 0.5, 0.25):
        assert abs(dr.keep_probability(p) - (1 - p)) <= 2.0 ** -17
        assert abs(dr.scale(p) * dr.keep_probability(p) - 1.0) <= 2.0 ** -23   # the scale is the inverse of the ACTUAL keep probability, rounded to fp32


def _site_elements(case, layer, site):
    nq, nk = ((case.N0, case.N0), (case.N1, case.N1), (case.N0, case.N1), (case.N1, case.N0))[layer]
    return case.B * nq * (sc.NHEAD * nk if site == 0 else case.F if site == 2 else case.C)


@pytest.mark.parametrize("gid", tuple(dr.GOLDENS))
def test_kept_fraction_per_site_is_within_four_sigma(gid):
    name, p, seed = dr.GOLDENS[gid]
    g = dr.load_golden(GOLDEN, gid)
    assert float(g["p"]) == p and int(g["seed"]) == seed and g["kept"].shape == (4, 4)
    kp = dr.keep_probability(p)
    for layer in range(4):
        for site in range(4):
            n = _site_elements(sc.CASES[name], layer, site)
            assert abs(g["kept"][layer, site] - kp) <= 4 * math.sqrt(kp * (1 - kp) / n), (layer, site, n, g["kept"][layer, site])
    if name == "small":   # the recorded fractions are those of the restated masks
        c = sc.CASES[name]
        for layer, (nq, nk) in enumerate(((c.N0, c.N0), (c.N1, c.N1), (c.N0, c.N1), (c.N1, c.N0))):
            ms = dr.layer_masks(seed, p, layer, c.B, nq, nk, c.C, c.F)
            assert [m.mean() for m in ms] == list(g["kept"][layer])


def test_masks_of_different_layers_sites_heads_and_seeds_differ():
    """Two independent masks agree with probability (1 - p)^2 + p^2 (0.5 at p = 0.5), not 1: within 4 sigma over n elements."""
    p, seed, B, Nq, Nk = 0.5, 77, 2, 64, 96
    a = dr.attn_mask(seed, p, 0, B, Nq, Nk)
    n = Nq * Nk
    tol = 4 * math.sqrt(0.25 / n)
    others = [a[0, 1], a[1, 0], dr.attn_mask(seed, p, 1, B, Nq, Nk)[0, 0], dr.attn_mask(seed + 1, p, 0, B, Nq, Nk)[0, 0],
              dr.attn_mask(seed + (1 << 32), p, 0, B, Nq, Nk)[0, 0], a[0, 2]]
    for o in others:
        assert abs((a[0, 0] == o).mean() - 0.5) <= tol
    r = [dr.row_mask(seed, p, layer, site, 1, 128, 64) for layer in (0, 1) for site in (1, 2, 3)]
    for i in range(len(r)):
        for j in range(i):
            assert abs((r[i] == r[j]).mean() - 0.5) <= 4 * math.sqrt(0.25 / r[i].size), (i, j)
    # neighbouring elements share a generator call and still differ: rows 4 k .. 4 k + 3 and columns 2 k, 2 k + 1 come from one call
    m = dr.row_mask(seed, p, 0, 1, 1, 128, 64)[0]
    assert abs((m[0::2] == m[1::2]).mean() - 0.5) <= 4 * math.sqrt(0.25 / (m.size / 2))
    assert abs((m[:, 0::2] == m[:, 1::2]).mean() - 0.5) <= 4 * math.sqrt(0.25 / (m.size / 2))


def test_mask_does_not_depend_on_how_the_call_is_cut():
    p, seed = 0.1, 0x1234567890
    full = dr.attn_mask(seed, p, 2, 3, 70, 130)
    assert np.array_equal(dr.attn_mask(seed, p, 2, 3, 70, 130, b=[1, 2]), full[1:])                    # batch items keep their masks
    assert np.array_equal(dr.attn_mask(seed, p, 2, 2, 33, 65), full[:2, :, :33, :65])                   # a shorter call is a corner of the longer one
    assert np.array_equal(dr.attn_mask(seed, p, 2, 3, 70, 130, q=np.arange(37, 70), k=np.arange(64, 130)), full[:, :, 37:, 64:])
    rows = dr.row_mask(seed, p, 2, 3, 3, 70, 64)
    assert np.array_equal(dr.row_mask(seed, p, 2, 3, 3, 70, 64, rows=np.arange(100, 150)), rows.reshape(210, 64)[100:150])
    assert np.array_equal(dr.row_mask(seed, p, 2, 3, 1, 70, 32), rows[:1, :, :32])                      # the first item's rows, fewer columns
    assert np.array_equal(dr.row_mask(seed, 0.5, 2, 3, 3, 70, 64) & rows, dr.row_mask(seed, 0.5, 2, 3, 3, 70, 64))   # one field, two thresholds: nested masks


@pytest.mark.parametrize("gid", tuple(dr.GOLDENS))
def test_goldens_load_and_equal_the_restatement(gid):
    """As tests/test_sct_train_cpu.py: the files hold the fp32 rounding (2^-24 of each element) of the reference's fp64 results, which the restatement meets to
    1e-9 of a tensor's largest magnitude (tools/gen_sct_dropout_golden.py asserts that): |golden - restatement| <= 1e-9 max |.| + 2^-24 |element|."""
    name, p, seed = dr.GOLDENS[gid]
    g = dr.load_golden(GOLDEN, gid)
    r = dr.grads(stc.make_case(name), p, seed)
    assert abs(float(g["L"]) - r["L"]) <= 1e-9 * max(1.0, abs(r["L"]))
    assert all(r[n] is None for n in stc.UNUSED) and len(KEYS) == 2 + 52
    for k in KEYS:
        a, b = g[stc.key(k)], r[k]
        assert a.dtype == np.float32 and a.shape == b.shape, k
        assert (np.abs(a.astype(np.float64) - b) <= 1e-9 * np.abs(b).max() + 2.0 ** -24 * np.abs(b)).all(), k
        assert float(g["dev_" + stc.key(k)]) <= 3e-5, k


def test_a_dropped_single_key_gives_a_zero_attention_row():
    """`swap` (N1 = 1): layers 1 and 2 have one key, so a dropped probability leaves nothing of the attention — the golden's seed has such rows and such that are kept."""
    name, p, seed = dr.GOLDENS["swap"]
    c = sc.CASES[name]
    m = dr.attn_mask(seed, p, 2, c.B, c.N0, 1)
    assert not m.all() and m.any()


def test_arguments_are_validated_before_anything_is_dereferenced():
    """No GPU needed: the pointers are host buffers (or null) that a correct library never reads.  The dropout entry points check what the calls they extend
    check, in that order, then p."""
    lib = _lib.load()
    assert lib.nl_abi_version() == 13
    buf = (ct.c_char * 8192)()
    p = ct.c_void_p((ct.addressof(buf) + 255) // 256 * 256)
    q = ct.c_void_p(p.value + 4)
    p2 = ct.c_void_p(p.value + 4096)
    ws_f, sb, wb = lib.nl_sct_workspace_bytes(2, 5, 7, 64, 128), lib.nl_sct_train_state_bytes(2, 5, 7, 64, 128), lib.nl_sct_backward_workspace_bytes(2, 5, 7, 64, 128)
    lwb = lib.nl_sct_layer_backward_workspace_bytes(2, 5, 7, 64, 128)
    OK, BAD, UNS, WS = _lib.NL_OK, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    grads = (ct.c_void_p * 52)(*([p.value] * 52))
    odd = (ct.c_void_p * 52)(*([p.value] * 51 + [q.value]))
    lgrads = (ct.c_void_p * 14)(*([p.value] * 14))
    bad_p = float("nan")   # every call below is refused by another argument too, or has this p: nothing may be launched

    def fwd(packed=p, C=64, nhead=8, F=128, prec=1, v0=p, pos0=p, N0=5, v1=p, pos1=p, N1=7, B=2, out0=p, out1=p2, state=p, state_bytes=sb, ws=p, ws_bytes=ws_f,
            dp=bad_p, seed=3):
        return lib.nl_sct_forward_train_dropout(packed, C, nhead, F, prec, v0, pos0, N0, v1, pos1, N1, B, out0, out1, state, state_bytes, ws, ws_bytes, dp, seed, None)

    def bwd(packed=p, tp=p, C=64, nhead=8, F=128, prec=1, v0=p, pos0=p, N0=5, v1=p, pos1=p, N1=7, B=2, state=p, state_bytes=sb, g0=p, g1=p, gv0=p, gp0=p, gv1=p,
            gp1=p, grads=grads, n=52, ws=p, ws_bytes=wb, dp=bad_p, seed=3):
        return lib.nl_sct_backward_dropout(packed, tp, C, nhead, F, prec, v0, pos0, N0, v1, pos1, N1, B, state, state_bytes, g0, g1, gv0, gp0, gv1, gp1, grads, n, ws,
                                           ws_bytes, dp, seed, None)

    def lay(packed=p, tp=p, C=64, nhead=8, F=128, l=2, prec=1, x=p, xp=p, Nq=5, mem=p, mp=p, Nk=7, B=2, g=p, gx=p, gxp=p, gm=p, gmp=p, grads=lgrads, n=14, ws=p,
            ws_bytes=lwb, dp=bad_p, seed=3):
        return lib.nl_sct_layer_backward_dropout(packed, tp, C, nhead, F, l, prec, x, xp, Nq, mem, mp, Nk, B, g, gx, gxp, gm, gmp, grads, n, ws, ws_bytes, dp, seed, None)

    for call in (fwd, bwd, lay):
        for dp in (-0.1, 1.0, float("nan"), 1.5, float("inf")):
            assert call(dp=dp) == BAD
        # the other arguments are refused first, with a good p and with a bad one
        for dp in (0.1, bad_p):
            assert call(ws=None, dp=dp) == WS and call(ws_bytes=16, dp=dp) == WS and call(ws=q, dp=dp) == WS
            assert call(packed=None, dp=dp) == BAD and call(packed=q, dp=dp) == BAD
            assert call(B=-1, dp=dp) == BAD and call(prec=7, dp=dp) == BAD
            assert call(prec=_lib.PREC_F16MX, dp=dp) == UNS
            assert call(nhead=4, dp=dp) == UNS and call(C=96, dp=dp) == UNS and call(F=520, dp=dp) == UNS
            assert call(B=0, ws=None, packed=None, dp=dp) == OK   # nothing to do, nothing touched
    assert fwd(N0=0) == BAD and fwd(v0=None) == BAD and fwd(out1=None) == BAD and fwd(out0=q) == BAD and fwd(B=1 << 20, N0=1 << 10) == UNS
    assert fwd(state=None, dp=0.1) == WS and fwd(state_bytes=sb - 1, dp=0.1) == WS and fwd(state=q, dp=0.1) == WS
    assert bwd(tp=None, dp=0.1) == BAD and bwd(N1=0, dp=0.1) == BAD and bwd(v1=q, dp=0.1) == BAD and bwd(grads=odd, dp=0.1) == BAD and bwd(n=48, dp=0.1) == BAD
    assert bwd(state_bytes=sb - 1, dp=0.1) == WS and bwd(ws_bytes=wb - 1, dp=0.1) == WS
    assert lay(l=4, dp=0.1) == BAD and lay(n=12, dp=0.1) == BAD and lay(ws_bytes=lwb - 1, dp=0.1) == WS
    assert lay(l=0, Nk=5, mem=None, mp=None, n=12, dp=0.1) == BAD   # a self layer has no memory-side gradient of its own

    def mask(seed=3, dp=0.1, layer=0, site=0, B=2, Nq=5, n=7, out=p):
        return lib.nl_sct_dropout_mask(seed, dp, layer, site, B, Nq, n, out, None)

    assert mask(layer=4) == BAD and mask(layer=-1) == BAD and mask(site=4) == BAD and mask(site=-1) == BAD and mask(B=-1) == BAD and mask(Nq=0) == BAD
    assert mask(n=0) == BAD and mask(out=None) == BAD and mask(B=1 << 20, Nq=1 << 10) == UNS and mask(B=0, out=None) == OK
    for dp in (-0.1, 1.0, float("nan")):
        assert mask(dp=dp) == BAD


def test_hip_dropout_on_cpu_tensors_takes_the_eager_path():
    from nerf_loc_amd.transformer import SelfCrossTransformer
    c = stc.make_case("small")
    case = c["case"]
    m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    assert m.hip_dropout is False and m.dropout_seed is None and m.dropout == 0.1
    m.train()
    m.hip_training = m.hip_dropout = True
    m.dropout_seed = 5
    o0, _ = m(*[torch.from_numpy(c[k]) for k in ("v0", "pos0", "v1", "pos1")])
    assert o0.requires_grad and m.pack_count == 0 and m._train_cache.pack_count == 0
