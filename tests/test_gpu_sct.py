"""GPU tests of SelfCrossTransformer in the HIP library (csrc/sct.hip through nl_sct_forward / nl_sct_layer and nerf_loc_amd.transformer): the reference's goldens,
every layer against the fp64 restatement, key / query tails, bit-for-bit invariance to the number of rows and batch items, the module path and its weight cache, and
the chain into the fine matcher.  The bar of the parity modes: max |error| <= 1e-4 x max |reference| per output."""
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_ref as sr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")   # the modes held to the bar (bf16: throughput mode, not held)
BAR = 1e-4
DEV = "cuda:0"

_CACHE = {}


def _case(name):
    """Recipe, golden and the fp64 restatement's four layer outputs: computed once per session, never modified."""
    if name not in _CACHE:
        c = sc.make_case(name)
        _CACHE[name] = (c, sc.load_golden(GOLDEN, name), sr.forward(c, torch.float64))
    return _CACHE[name]


def _module(c, mode="bf16x3", **kw):
    from nerf_loc_amd.transformer import SelfCrossTransformer
    case = c["case"]
    m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, precision=mode, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    return m.to(DEV).eval()


def _packed(name):
    key = ("packed", name)
    if key not in _CACHE:
        m = _module(_case(name)[0])
        _CACHE[key] = (m, m._pack(torch.device(DEV)))
    return _CACHE[key][1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _lib_forward(name, mode, v0, pos0, v1, pos1):
    """nl_sct_forward called directly on numpy inputs."""
    case = sc.CASES[name]
    lib = _lib.load()
    t = [_dev(a) for a in (v0, pos0, v1, pos1)]
    B, N0, N1 = t[0].shape[0], t[0].shape[1], t[2].shape[1]
    o0 = torch.empty((B, N0, case.C), dtype=torch.float32, device=DEV)
    o1 = torch.empty((B, N1, case.C), dtype=torch.float32, device=DEV)
    need = lib.nl_sct_workspace_bytes(B, N0, N1, case.C, case.F)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.nl_sct_forward(_packed(name).data_ptr(), case.C, sc.NHEAD, case.F, _lib.PRECISIONS[mode], t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(),
                                  t[3].data_ptr(), N1, B, o0.data_ptr(), o1.data_ptr(), ws.data_ptr(), need, st), "nl_sct_forward")
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy()


def _lib_layer(name, mode, l, x, px, mem, pm):
    """nl_sct_layer called directly on numpy inputs."""
    case = sc.CASES[name]
    lib = _lib.load()
    tx, tpx = _dev(x), _dev(px)
    tm, tpm = (tx, tpx) if l < 2 else (_dev(mem), _dev(pm))
    B, Nq, Nk = tx.shape[0], tx.shape[1], tm.shape[1]
    out = torch.empty((B, Nq, case.C), dtype=torch.float32, device=DEV)
    need = lib.nl_sct_workspace_bytes(B, Nq, Nk, case.C, case.F)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.nl_sct_layer(_packed(name).data_ptr(), case.C, sc.NHEAD, case.F, l, _lib.PRECISIONS[mode], tx.data_ptr(), tpx.data_ptr(), Nq, tm.data_ptr(),
                                tpm.data_ptr(), Nk, B, out.data_ptr(), ws.data_ptr(), need, st), "nl_sct_layer")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rel(a, ref):
    assert np.isfinite(a).all()
    return float(np.abs(a.astype(np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sc.GOLDEN_CASES)
def test_forward_against_the_golden(name, mode):
    c, g, _ = _case(name)
    o0, o1 = _lib_forward(name, mode, c["v0"], c["pos0"], c["v1"], c["pos1"])
    e0, e1 = _rel(o0, g["out0"]), _rel(o1, g["out1"])
    print(f"sct forward {name} {mode}: max |error| / max |reference| out0 {e0:.2e} out1 {e1:.2e} (reference fp32 vs fp64 {float(g['ref_fp32_vs_fp64'].max()):.2e})")
    assert e0 <= BAR and e1 <= BAR


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("c192", "fine", "peaked"))
def test_each_layer_against_the_fp64_restatement(name, mode):
    c, _, outs = _case(name)
    errs = []
    for l in range(4):
        x, px, mem, pm = sr.layer_inputs(c, outs, l)   # the restatement's own intermediates: an error belongs to its layer
        errs.append(_rel(_lib_layer(name, mode, l, x, px, mem, pm), outs[l]))
    print(f"sct layers {name} {mode}: " + " ".join(f"layer {l} {e:.2e}" for l, e in enumerate(errs)))
    assert max(errs) <= BAR, errs


@pytest.mark.parametrize("mode", MODES)
def test_key_and_query_tails(mode):
    c, _, outs = _case("long")
    x, px, mem, pm = sr.layer_inputs(c, outs, 2)
    worst = 0.0
    for nq in (1, 33, 130):
        for nk in (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 1100):
            a = (x[:, :nq], px[:, :nq], mem[:, :nk], pm[:, :nk])
            ref = sr.layer(c["state"], 2, *a, dtype=torch.float64)
            e = _rel(_lib_layer("long", mode, 2, *a), ref)
            worst = max(worst, e)
            assert e <= BAR, (nq, nk, e)
    print(f"sct tails {mode}: worst max |error| / max |reference| over 33 (Nq, Nk) cuts {worst:.2e}")


# ------------------------------------------------------------------------------------------ invariance, bit for bit
@pytest.mark.parametrize("mode", MODES + ("bf16",))
def test_a_query_row_does_not_depend_on_the_rows_around_it(mode):
    c, _, outs = _case("long")
    x, px, mem, pm = sr.layer_inputs(c, outs, 2)
    row = 45
    full = _lib_layer("long", mode, 2, x, px, mem, pm)[:, row]
    part = _lib_layer("long", mode, 2, x[:, 40:90], px[:, 40:90], mem, pm)[:, row - 40]   # a slice that starts inside a 32-row tile
    alone = _lib_layer("long", mode, 2, x[:, row:row + 1], px[:, row:row + 1], mem, pm)[:, 0]
    assert np.array_equal(full, part) and np.array_equal(full, alone)


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_item_does_not_depend_on_the_batch(mode):
    c, _, _ = _case("fine64")
    ins = [c[k] for k in ("v0", "pos0", "v1", "pos1")]
    B, i = c["case"].B, 7
    f0, f1 = _lib_forward("fine64", mode, *ins)
    a0, a1 = _lib_forward("fine64", mode, *[a[i:i + 1] for a in ins])
    perm = np.arange(B)[::-1].copy()
    p0, p1 = _lib_forward("fine64", mode, *[a[perm] for a in ins])
    assert np.array_equal(f0[i], a0[0]) and np.array_equal(f1[i], a1[0])
    assert np.array_equal(f0, p0[perm]) and np.array_equal(f1, p1[perm])


def test_forward_twice_gives_the_same_bits():
    c, _, _ = _case("c192")
    ins = [c[k] for k in ("v0", "pos0", "v1", "pos1")]
    a, b = _lib_forward("c192", "bf16x3", *ins), _lib_forward("c192", "bf16x3", *ins)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ through the module
def test_module_equals_the_library_call_and_caches_its_weights():
    c, g, _ = _case("c128")
    m = _module(c)
    ins = [_dev(c[k]) for k in ("v0", "pos0", "v1", "pos1")]
    with torch.no_grad():
        o0, o1 = m(*ins)
        m(*ins)
    assert m.pack_count == 1 and o0.is_contiguous() and o1.is_contiguous()
    d0, d1 = _lib_forward("c128", "bf16x3", c["v0"], c["pos0"], c["v1"], c["pos1"])
    assert np.array_equal(o0.cpu().numpy(), d0) and np.array_equal(o1.cpu().numpy(), d1)
    with torch.no_grad():
        m.cross_attn_layer1.linear2.bias.add_(0.5)   # in place: the same storage, a new version
        q0, q1 = m(*ins)
    assert m.pack_count == 2
    assert not np.array_equal(q1.cpu().numpy(), d1)
    # transposed views are accepted (one copy)
    with torch.no_grad():
        m.cross_attn_layer1.linear2.bias.sub_(0.5)
        tv = [t.transpose(0, 1).contiguous().transpose(0, 1) for t in ins]
        assert not tv[0].is_contiguous()
        r0, r1 = m(*tv)
    assert _rel(r0.cpu().numpy(), g["out0"]) <= BAR and _rel(r1.cpu().numpy(), g["out1"]) <= BAR
    # B = 0
    with torch.no_grad():
        z0, z1 = m(*[t[:0] for t in ins])
    assert tuple(z0.shape) == (0, c["case"].N0, c["case"].C) and tuple(z1.shape) == (0, c["case"].N1, c["case"].C)


def test_unsupported_configuration_raises_where_it_is_used():
    from nerf_loc_amd.transformer import SelfCrossTransformer
    m = SelfCrossTransformer(d_model=96, nhead=8, dim_feedforward=128).to(DEV).eval()
    x = torch.zeros(1, 3, 96, device=DEV)
    with torch.no_grad(), pytest.raises(RuntimeError, match="nhead == 8"):
        m(x, x, x, x)


def test_throughput_mode_runs():
    c, g, _ = _case("c192")
    m = _module(c, mode="bf16")
    with torch.no_grad():
        o0, o1 = m(*[_dev(c[k]) for k in ("v0", "pos0", "v1", "pos1")])
    e0, e1 = _rel(o0.cpu().numpy(), g["out0"]), _rel(o1.cpu().numpy(), g["out1"])
    print(f"sct forward c192 bf16 (not held to the bar): out0 {e0:.2e} out1 {e1:.2e}")


def test_training_mode_on_the_gpu_takes_the_eager_path():
    c, g, _ = _case("small")
    m = _module(c, dropout=0.0).train()
    o0, o1 = m(*[_dev(c[k]) for k in ("v0", "pos0", "v1", "pos1")])
    assert o0.requires_grad and m.pack_count == 0
    e0, e1 = _rel(o0.detach().cpu().numpy(), g["out0"]), _rel(o1.detach().cpu().numpy(), g["out1"])
    print(f"sct eager on the GPU, small: out0 {e0:.2e} out1 {e1:.2e}")
    assert e0 <= BAR and e1 <= BAR


# ------------------------------------------------------------------------------------------ chain into the fine matcher
def test_chain_into_fine_matching():
    from nerf_loc_amd.fine_matching import FineMatching
    from tests import fine_cases as fc
    c, g, _ = _case("fine")
    fcase = fc.make_case("c192")
    fm = FineMatching(fc.matching_config(fcase["case"]), precision="bf16x3")
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in fcase["mlp"].items()}, strict=True)
    fm = fm.to(DEV).eval()
    m = _module(c)
    M = c["case"].B
    kc = torch.zeros((M, 2), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        o0, o1 = m(*[_dev(c[k]) for k in ("v0", "pos0", "v1", "pos1")])
        ours = fm.match(o0[:, 0], o1, kc)[0].cpu().numpy()
        ref = fm.match(_dev(g["out0"])[:, 0], _dev(g["out1"]), kc)[0].cpu().numpy()
    d = float(np.abs(ours - ref).max())
    print(f"sct -> FineMatching chain: max |expec_f difference| {d:.2e}")
    assert np.isfinite(ours).all() and d <= 1e-3
