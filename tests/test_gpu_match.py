"""GPU tests of the coarse matcher (csrc/s2d.hip through nl_s2d_match and nerf_loc_amd.matching.S2DMatching): scores against the reference's goldens and
against the fp64 restatement, exact selection on the kernel's own scores, matches against the reference on decided rows, invariance, workspace / guard
behaviour and the module path."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import match_cases as mc
from tests import match_ref as mr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")          # the modes held to the parity bar (f16mx: NL_ERR_UNSUPPORTED for this kernel; bf16: throughput mode, not held)
BAR = 1e-4
EPS = 2e-4
DEV = "cuda:0"


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"s2d_{name}.npz"))


def _module(c, mode, **kw):
    from nerf_loc_amd.matching import S2DMatching
    m = S2DMatching(c["case"].C, thr=c["thr"], precision=mode, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    return m.to(DEV).eval()


def _run(c, mode, desc0=None, desc1=None, want=True, module=None):
    m = module or _module(c, mode)
    d0 = torch.from_numpy(c["desc0"] if desc0 is None else desc0).to(DEV)
    d1 = torch.from_numpy(c["desc1"] if desc1 is None else desc1).to(DEV)
    s, mj, ms = m.match(d0, d1, want_scores=want)
    torch.cuda.synchronize()
    return (s.cpu().numpy() if s is not None else None), mj.cpu().numpy().astype(np.int64), ms.cpu().numpy()


_FP64 = {}


def _fp64_scores(name, c):
    if name not in _FP64:   # the shipped size costs 0.4 TFLOP of fp64 on the CPU: once per session, not once per mode
        _FP64[name] = mr.scores(c["desc0"], c["desc1"], c["weights"], torch.float64, chunk=32)
    return _FP64[name]


def _errs(s, ref):
    a, b = s.astype(np.float64), ref.astype(np.float64)
    return np.abs(a - b).max() / np.abs(b).max(), np.linalg.norm(a - b) / np.linalg.norm(b)


# ------------------------------------------------------------------------------------------ 3. scores
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", mc.GOLDEN_CASES)
def test_scores_against_the_reference_goldens(name, mode):
    c, g = mc.make_case(name), _golden(name)
    s, _, _ = _run(c, mode)
    emax, el2 = _errs(s, g["score_matrix"])
    print(f"s2d scores {name} {mode}: max-rel {emax:.3e} l2-rel {el2:.3e}")
    assert emax <= BAR and el2 <= BAR


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("mid", "full"))
def test_scores_against_fp64_at_the_large_shapes(name, mode):
    """(256, 1200) and the shipped size (1024, 4800), C = 192, against tests/match_ref.py in fp64 (32-row chunks)."""
    c = mc.make_case(name)
    s, mj, _ = _run(c, mode)
    ref = _fp64_scores(name, c)
    emax, el2 = _errs(s, ref)
    print(f"s2d scores {name} {mode}: max-rel {emax:.3e} l2-rel {el2:.3e}")
    assert emax <= BAR and el2 <= BAR
    # selection on the kernel's own scores (test 4) and against the fp64 reference on decided rows (test 5) at these sizes too
    assert np.array_equal(mj, mr.select(s, c["thr"]))
    und = mr.undecided_rows(ref, c["thr"], EPS)
    print(f"s2d {name}: {int(und.sum())} undecided rows of {len(und)}")
    assert und.sum() <= 0.01 * len(und)
    assert np.array_equal(mj[~und], mr.select(ref, c["thr"])[~und])


def test_f16mx_is_refused_for_the_matcher():
    c = mc.make_case("c128")
    with pytest.raises(RuntimeError, match="unsupported"):
        _run(c, "f16mx")


# ------------------------------------------------------------------------------------------ 4. selection is exact on the kernel's own scores
@pytest.mark.parametrize("mode", MODES + ("bf16",))
@pytest.mark.parametrize("name", mc.GOLDEN_CASES)
def test_selection_is_exact_on_the_kernels_own_scores(name, mode):
    c = mc.make_case(name)
    s, mj, ms = _run(c, mode)
    want = mr.select(s, c["thr"])
    assert np.array_equal(mj, want)
    assert np.array_equal(ms[want >= 0], s[np.nonzero(want >= 0)[0], want[want >= 0]]) and not ms[want < 0].any()
    # thr exactly at one of the row maxima: strict `>` drops that row (and whatever else sits at or below it)
    rows = np.nonzero(want >= 0)[0]
    thr = float(s[rows[len(rows) // 2]].max())
    m = _module(c, mode)
    m.thr = thr
    s2, mj2, _ = _run(c, mode, module=m)
    assert np.array_equal(s2, s)
    assert np.array_equal(mj2, mr.select(s, np.float32(thr))) and mj2[rows[len(rows) // 2]] == -1
    if name == "ties":
        assert (s[7] == np.float32(1.0)).sum() >= 2 and np.array_equal(s[:, 10], s[:, 11]) and np.array_equal(s[20], s[21])
        assert mj[5] == 10 and mj[20] == mj[21] >= 0


# ------------------------------------------------------------------------------------------ 5. matches against the reference
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("small", "c128", "c256"))
def test_matches_equal_the_reference_on_decided_rows(name, mode):
    c, g = mc.make_case(name), _golden(name)
    und = mr.undecided_rows(g["score_matrix"], c["thr"], EPS)
    assert und.sum() <= 0.01 * len(und), "the recipe has too many undecided rows: change its seed"
    ref_j = np.full(c["case"].N, -1, dtype=np.int64)
    ref_j[g["i_ids"]] = g["j_ids"]
    _, mj, _ = _run(c, mode)
    assert np.array_equal(mj[~und], ref_j[~und])


# ------------------------------------------------------------------------------------------ 6. invariance
@pytest.mark.parametrize("mode", MODES)
def test_scores_do_not_depend_on_position_or_shape(mode):
    c = mc.make_case("small")
    m = _module(c, mode)
    s, mj, _ = _run(c, mode, module=m)
    s_again, mj_again, _ = _run(c, mode, module=m)
    assert np.array_equal(s, s_again) and np.array_equal(mj, mj_again)                 # two calls: the same bits
    for a, b in ((0, 1), (5, 38), (33, 96), (17, 18)):                                 # rows [a, b) alone
        sa, _, _ = _run(c, mode, desc0=c["desc0"][a:b], module=m)
        assert np.array_equal(sa, s[a:b]), (a, b)
    for a, b in ((0, 1), (7, 40), (31, 600), (95, 161), (599, 600)):                   # columns [a, b) alone
        sa, _, _ = _run(c, mode, desc1=c["desc1"][a:b], module=m)
        assert np.array_equal(sa, s[:, a:b]), (a, b)
    for n, k in ((1, 1), (1, 33), (31, 31), (33, 65), (32, 64), (63, 97), (65, 127)):  # N and M one off every tile multiple
        sa, mja, _ = _run(c, mode, desc0=c["desc0"][:n], desc1=c["desc1"][:k], module=m)
        assert np.array_equal(sa, s[:n, :k]), (n, k)
        assert np.array_equal(mja, mr.select(sa, c["thr"]))


def test_side_stream_call_gives_the_same_bits():
    c = mc.make_case("small")
    m = _module(c, "bf16x3")
    s, mj, _ = _run(c, "bf16x3", module=m)
    d0, d1 = torch.from_numpy(c["desc0"]).to(DEV), torch.from_numpy(c["desc1"]).to(DEV)
    big = mc.make_case("mid")
    mb = _module(big, "bf16x3")
    b0, b1 = torch.from_numpy(big["desc0"]).to(DEV), torch.from_numpy(big["desc1"]).to(DEV)
    mb.match(b0, b1)                                   # packs mb's weights
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    sb0, _, _ = mb.match(b0, b1)                       # default stream: keeps the device busy ...
    with torch.cuda.stream(side):                      # ... while the side stream runs the small case
        s2, mj2, _ = m.match(d0, d1)
    sb1, _, _ = mb.match(b0, b1)
    torch.cuda.synchronize()
    assert np.array_equal(s2.cpu().numpy(), s) and np.array_equal(mj2.cpu().numpy().astype(np.int64), mj)
    assert torch.equal(sb0, sb1)


# ------------------------------------------------------------------------------------------ 7. workspace, optional output, guards
@pytest.mark.parametrize("mode", MODES)
def test_without_score_matrix_the_matches_are_the_same(mode):
    c = mc.make_case("small")
    s, mj, ms = _run(c, mode)
    s0, mj0, ms0 = _run(c, mode, want=False)
    assert s0 is None and np.array_equal(mj0, mj) and np.array_equal(ms0, ms)


@pytest.mark.parametrize("want", (True, False))
def test_workspace_query_is_honoured_and_guards_stay_intact(want):
    """Every buffer is EXACTLY its queried / documented size with 0xA5 canaries before and behind it; one byte short is NL_ERR_WORKSPACE with nothing launched."""
    c = mc.make_case("small")
    case = c["case"]
    N, M, C = case.N - 1, case.M - 3, case.C           # ragged in both directions
    lib = _lib.load()
    m = _module(c, "bf16x3")
    packed = m._packed_weights(torch.device(DEV))
    G = 4096

    def guarded(nbytes):
        buf = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        return buf, buf[G:G + nbytes]
    d0 = torch.from_numpy(c["desc0"][:N]).to(DEV).contiguous()
    d1 = torch.from_numpy(c["desc1"][:M]).to(DEV).contiguous()
    need = lib.nl_s2d_min_workspace_bytes(N, M, C, int(want))
    bufs = {"ws": guarded(need), "mj": guarded(N * 4), "ms": guarded(N * 4)}
    if want:
        bufs["s"] = guarded(N * M * 4)
    st = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes):
        return lib.nl_s2d_match(packed.data_ptr(), C, _lib.PREC_BF16X3, d0.data_ptr(), N, d1.data_ptr(), M, ct.c_float(c["thr"]),
                                bufs["s"][1].data_ptr() if want else None, bufs["mj"][1].data_ptr(), bufs["ms"][1].data_ptr(), bufs["ws"][1].data_ptr(), ws_bytes, st)
    assert call(need - 1) == _lib.NL_ERR_WORKSPACE
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf == 0xA5).all()), f"{k}: written although the call was refused"
    assert call(need) == _lib.NL_OK
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        n = view.numel()
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + n:] == 0xA5).all()), f"{k}: guard bytes overwritten"
    mj = bufs["mj"][1].view(torch.int32).cpu().numpy().astype(np.int64)
    s_ref, mj_ref, _ = _run(c, "bf16x3", desc0=c["desc0"][:N], desc1=c["desc1"][:M], module=m)
    assert np.array_equal(mj, mj_ref)
    if want:
        assert np.array_equal(bufs["s"][1].view(torch.float32).reshape(N, M).cpu().numpy(), s_ref)


# ------------------------------------------------------------------------------------------ 8. through the module
def test_module_forward_fills_data_like_the_reference_and_repacks_on_change():
    c, g = mc.make_case("small"), _golden("small")
    m = _module(c, "bf16x3")
    d0, d1 = torch.from_numpy(c["desc0"]).to(DEV), torch.from_numpy(c["desc1"]).to(DEV)
    data = {"kept": 1}
    with torch.no_grad():
        out = m(d0, d1, data)
    assert out is data and data["kept"] == 1
    assert data["i_ids"].dtype == torch.int64 and data["j_ids"].dtype == torch.int64 and data["score_matrix"].dtype == torch.float32
    assert data["i_ids"].device == d0.device and data["score_matrix"].shape == (96, 600)
    i_ids, j_ids = data["i_ids"].cpu().numpy(), data["j_ids"].cpu().numpy()
    assert np.all(np.diff(i_ids) > 0)
    assert np.array_equal(i_ids, g["i_ids"]) and np.array_equal(j_ids, g["j_ids"])      # the small case has no undecided row (asserted in test 5)
    assert m.pack_count == 1
    m(d0, d1, {})
    assert m.pack_count == 1                                                            # cached
    with torch.no_grad():
        m.mlps[4].bias.add_(1.0)                                                        # in place: _version changes
    data2 = m(d0, d1, {})
    assert m.pack_count == 2
    want = mr.scores(c["desc0"], c["desc1"], {**c["weights"], "mlps.4.bias": c["weights"]["mlps.4.bias"] + np.float32(1.0)}, torch.float64)
    emax, _ = _errs(data2["score_matrix"].cpu().numpy(), want)
    assert emax <= BAR
    # want_score_matrix=False: the key is there and None
    m2 = _module(c, "bf16x3", want_score_matrix=False)
    d3 = m2(d0, d1, {})
    assert d3["score_matrix"] is None and np.array_equal(d3["i_ids"].cpu().numpy(), g["i_ids"]) and np.array_equal(d3["j_ids"].cpu().numpy(), g["j_ids"])
    # training mode on the device: the eager formulation, with the loss
    m.train()
    dt = m(d0, d1, {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"]).to(DEV)})
    assert dt["coarse_loss"].requires_grad and dt["score_matrix"].shape == (96, 600)
