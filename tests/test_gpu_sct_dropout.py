"""GPU tests of the SelfCrossTransformer training step with dropout inside the kernels (nl_sct_forward_train_dropout / nl_sct_backward_dropout /
nl_sct_layer_backward_dropout / nl_sct_dropout_mask and the module's hip_dropout path): the device masks against their numpy restatement, outputs and every
gradient against the reference's goldens with the library's masks (C = 64) or the fp64 restatement (C >= 128), each layer on its own, p == 0, determinism,
batch slicing, NULL outputs and the module.
The bar of the parity modes is the project's: per tensor, max |error| <= 1e-4 x max |reference|."""
import ctypes

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_dropout_ref as dr
from tests import sct_train_cases as stc
from tests import test_gpu_sct_train as base   # its helpers and caches (cases, packed images), never its tests

pytestmark = pytest.mark.gpu

GOLDEN = base.GOLDEN
MODES = base.MODES
BAR = 1e-4
DEV = base.DEV
INS = base.INS
OUTS = ("out0", "out1")

_CACHE = {}
_dev, _ptr, _rel, _worst, _case, _images = base._dev, base._ptr, base._rel, base._worst, base._case, base._images


def _spec(gid):
    return dr.GOLDENS[gid] if gid in dr.GOLDENS else dr.REF_CASES[gid]


def _ref(gid):
    """{tensor name: fp64-accurate array} of out0, out1 and the 52 gradients (loaded or computed once, never modified)."""
    if ("ref", gid) not in _CACHE:
        name, p, seed = _spec(gid)
        keys = OUTS + stc.INPUT_GRADS + stc.PARAM_NAMES
        if gid in dr.GOLDENS:
            g = dr.load_golden(GOLDEN, gid)
            r = {k: g[stc.key(k)] for k in keys}
        else:
            full = dr.grads(_case(name), p, seed)
            r = {k: full[k] for k in keys}
        _CACHE[("ref", gid)] = r
    return _CACHE[("ref", gid)]


def _step(name, mode, ins, g0, g1, p, seed, want_in=(True,) * 4, want_p=None, backward=True, plain=False):
    """nl_sct_forward_train_dropout (+ nl_sct_backward_dropout) on numpy inputs: (out0, out1, {name: gradient}); plain: the entry points without dropout."""
    case = sc.CASES[name]
    lib = _lib.load()
    C, F = case.C, case.F
    packed, tpacked = _images(name)
    t = [_dev(a) for a in ins]
    B, N0, N1 = t[0].shape[0], t[0].shape[1], t[2].shape[1]
    o0 = torch.empty((B, N0, C), dtype=torch.float32, device=DEV)
    o1 = torch.empty((B, N1, C), dtype=torch.float32, device=DEV)
    sb, wb = lib.nl_sct_train_state_bytes(B, N0, N1, C, F), lib.nl_sct_workspace_bytes(B, N0, N1, C, F)
    state, ws = torch.empty(sb, dtype=torch.uint8, device=DEV), torch.empty(wb, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    prec = _lib.PRECISIONS[mode]
    drop = () if plain else (p, seed)
    fwd, bwd = (lib.nl_sct_forward_train, lib.nl_sct_backward) if plain else (lib.nl_sct_forward_train_dropout, lib.nl_sct_backward_dropout)
    _lib.check(fwd(packed.data_ptr(), C, sc.NHEAD, F, prec, t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(), t[3].data_ptr(), N1, B, o0.data_ptr(), o1.data_ptr(),
                   state.data_ptr(), sb, ws.data_ptr(), wb, *drop, st), "forward")
    grads = {}
    if backward:
        gin = [torch.full_like(t[i], float("nan")) if want_in[i] else None for i in range(4)]
        shapes = [_case(name)["state"][n].shape for n in sc.STATE_NAMES]
        gpar = [torch.full(tuple(s), float("nan"), dtype=torch.float32, device=DEV) if n not in stc.UNUSED and (want_p is None or n in want_p) else None
                for n, s in zip(sc.STATE_NAMES, shapes)]
        arr = (ctypes.c_void_p * 52)(*[_ptr(g) for g in gpar])
        bb = lib.nl_sct_backward_workspace_bytes(B, N0, N1, C, F)
        bws = torch.empty(bb, dtype=torch.uint8, device=DEV)
        tg0, tg1 = (None if g is None else _dev(g) for g in (g0, g1))
        _lib.check(bwd(packed.data_ptr(), tpacked.data_ptr(), C, sc.NHEAD, F, prec, t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(), t[3].data_ptr(), N1, B,
                       state.data_ptr(), sb, _ptr(tg0), _ptr(tg1), _ptr(gin[0]), _ptr(gin[1]), _ptr(gin[2]), _ptr(gin[3]), arr, 52, bws.data_ptr(), bb, *drop, st),
                   "backward")
        torch.cuda.synchronize()
        grads = {k: g.cpu().numpy() for k, g in zip(stc.INPUT_GRADS, gin) if g is not None}
        grads.update({n: g.cpu().numpy() for n, g in zip(sc.STATE_NAMES, gpar) if g is not None})
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy(), grads


def _full_step(gid, mode, seed=None, **kw):
    name, p, s = _spec(gid)
    c = _case(name)
    return _step(name, mode, [c[k] for k in INS], c["g_out0"], c["g_out1"], p, s if seed is None else seed, **kw)


def _result(gid, mode):
    """One forward + backward per (fixture, mode), shared by the output and the gradient tests."""
    if ("res", gid, mode) not in _CACHE:
        o0, o1, grads = _full_step(gid, mode)
        _CACHE[("res", gid, mode)] = {"out0": o0, "out1": o1, **grads}
    return _CACHE[("res", gid, mode)]


# ------------------------------------------------------------------------------------------ the masks
def _device_mask(seed, p, layer, site, B, Nq, n):
    rows = B * Nq * (8 if site == 0 else 1)
    out = torch.full((rows, n), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().nl_sct_dropout_mask(seed, p, layer, site, B, Nq, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "nl_sct_dropout_mask")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("gid", ("small", "small_p50", "swap"))
def test_device_masks_equal_the_numpy_masks(gid):
    name, p, seed = dr.GOLDENS[gid]
    c = sc.CASES[name]
    for layer, (nq, nk) in enumerate(((c.N0, c.N0), (c.N1, c.N1), (c.N0, c.N1), (c.N1, c.N0))):
        want = dr.layer_masks(seed, p, layer, c.B, nq, nk, c.C, c.F)
        for site, n in enumerate((nk, c.C, c.F, c.C)):
            got = _device_mask(seed, p, layer, site, c.B, nq, n)
            assert set(np.unique(got)) <= {0, 1}
            assert np.array_equal(got.astype(bool), want[site].reshape(got.shape)), (layer, site)


def test_device_mask_of_the_long_attention_site():
    name, p, seed = dr.GOLDENS["long"]
    c = sc.CASES[name]
    got = _device_mask(seed, p, 2, 0, c.B, c.N0, c.N1)   # 130 queries x 1100 keys: four key ranges and a tail tile in the kernels, one function here
    assert np.array_equal(got.astype(bool), dr.attn_mask(seed, p, 2, c.B, c.N0, c.N1).reshape(got.shape))


# ------------------------------------------------------------------------------------------ against the reference with the library's masks
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gid", tuple(dr.GOLDENS) + tuple(dr.REF_CASES))
def test_outputs_against_the_reference(gid, mode):
    ref, got = _ref(gid), _result(gid, mode)
    errs = {k: _rel(got[k], ref[k]) for k in OUTS}
    print(f"sct dropout forward {gid} {mode}: max |error| / max |reference| out0 {errs['out0']:.2e} out1 {errs['out1']:.2e}")
    assert all(e <= BAR for e in errs.values()), errs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gid", tuple(dr.GOLDENS) + tuple(dr.REF_CASES))
def test_gradients_against_the_reference(gid, mode):
    ref = {k: v for k, v in _ref(gid).items() if k not in OUTS}
    got = {k: v for k, v in _result(gid, mode).items() if k not in OUTS}
    assert len(ref) == 4 + 48 and set(got) == set(ref)
    errs, k = _worst(got, ref)
    src = "golden" if gid in dr.GOLDENS else "fp64 restatement"
    print(f"sct dropout backward {gid} {mode} vs {src}: worst max |error| / max |reference| {errs[k]:.2e} ({k}); inputs " +
          " ".join(f"{n} {errs[n]:.2e}" for n in stc.INPUT_GRADS))
    bad = {n: e for n, e in errs.items() if e > BAR}
    assert not bad, bad


def test_throughput_mode_runs():
    got = _full_step("small", "bf16")
    errs, k = _worst(got[2], {n: v for n, v in _ref("small").items() if n not in OUTS})
    print(f"sct dropout backward small bf16 (not held to the bar): worst {errs[k]:.2e} ({k})")
    assert all(np.isfinite(g).all() for g in got[2].values())


# ------------------------------------------------------------------------------------------ one layer at a time
def _layer_backward(name, mode, l, x, px, mem, pm, g_out, p, seed):
    case = sc.CASES[name]
    lib = _lib.load()
    C, F = case.C, case.F
    packed, tpacked = _images(name)
    tx, tpx = _dev(x), _dev(px)
    cross = l >= 2
    tm, tpm = (_dev(mem), _dev(pm)) if cross else (None, None)
    B, Nq, Nk = tx.shape[0], tx.shape[1], (tm.shape[1] if cross else tx.shape[1])
    names = sc.layer_names(sc.LAYERS[l])
    gx, gpx = torch.full_like(tx, float("nan")), torch.full_like(tx, float("nan"))
    gm, gpm = (torch.full_like(tm, float("nan")), torch.full_like(tm, float("nan"))) if cross else (None, None)
    gpar = [None if n in stc.UNUSED else torch.full(_case(name)["state"][n].shape, float("nan"), dtype=torch.float32, device=DEV) for n in names]
    arr = (ctypes.c_void_p * len(names))(*[_ptr(g) for g in gpar])
    bb = lib.nl_sct_layer_backward_workspace_bytes(B, Nq, Nk, C, F)
    ws = torch.empty(bb, dtype=torch.uint8, device=DEV)
    tg = _dev(g_out)
    _lib.check(lib.nl_sct_layer_backward_dropout(packed.data_ptr(), tpacked.data_ptr(), C, sc.NHEAD, F, l, _lib.PRECISIONS[mode], tx.data_ptr(), tpx.data_ptr(), Nq,
                                                 _ptr(tm), _ptr(tpm), Nk, B, tg.data_ptr(), gx.data_ptr(), gpx.data_ptr(), _ptr(gm), _ptr(gpm), arr, len(names),
                                                 ws.data_ptr(), bb, p, seed, torch.cuda.current_stream().cuda_stream), "nl_sct_layer_backward_dropout")
    torch.cuda.synchronize()
    res = {"g_x": gx.cpu().numpy(), "g_pos_x": gpx.cpu().numpy()}
    if cross:
        res.update({"g_mem": gm.cpu().numpy(), "g_pos_mem": gpm.cpu().numpy()})
    res.update({n: g.cpu().numpy() for n, g in zip(names, gpar) if g is not None})
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gid", ("c192", "peaked", "swap"))
def test_each_layer_against_fp64_autograd(gid, mode):
    name, p, seed = _spec(gid)
    c = _case(name)
    if ("mid", gid) not in _CACHE:
        _CACHE[("mid", gid)] = dr.grads(c, p, seed)
    full = _CACHE[("mid", gid)]
    # the restatement's own intermediates: an error belongs to its layer
    inputs = ((c["v0"], c["pos0"], None, None), (c["v1"], c["pos1"], None, None), (full["mid0"], c["pos0"], full["mid1"], c["pos1"]),
              (full["mid1"], c["pos1"], full["out0"], c["pos0"]))
    worst = []
    for l, (x, px, mem, pm) in enumerate(inputs):
        g_out = c["g_out0"] if l in (0, 2) else c["g_out1"]
        ref = {k: v for k, v in dr.layer_grads(c, l, x, px, mem, pm, g_out, p, seed).items() if v is not None}
        got = _layer_backward(name, mode, l, x, px, mem, pm, g_out, p, seed)
        assert set(got) == set(ref)
        errs, k = _worst(got, ref)
        worst.append((errs[k], k))
        assert errs[k] <= BAR, (l, k, errs[k])
    print(f"sct dropout layer backward {gid} {mode}: " + " ".join(f"layer {l} {e:.2e} ({k.split('.', 1)[-1]})" for l, (e, k) in enumerate(worst)))


# ------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("mode", MODES + ("bf16",))
@pytest.mark.parametrize("name", ("small", "c128"))
def test_p_zero_has_the_bits_of_the_entry_points_without_dropout(name, mode):
    c = _case(name)
    ins = [c[k] for k in INS]
    a = _step(name, mode, ins, c["g_out0"], c["g_out1"], 0.0, 12345)
    b = _step(name, mode, ins, c["g_out0"], c["g_out1"], 0.0, 0, plain=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set(a[2]) == set(b[2]) and len(a[2]) == 52 and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("mode", MODES + ("bf16",))
def test_one_seed_gives_the_same_bits_and_two_seeds_differ(mode):
    a, b = _full_step("c128", mode), _full_step("c128", mode)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set(a[2]) == set(b[2]) and len(a[2]) == 52 and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    o = _full_step("c128", mode, seed=_spec("c128")[2] + 1)
    assert not np.array_equal(a[0], o[0]) and not np.array_equal(a[1], o[1]) and not np.array_equal(a[2]["g_v0"], o[2]["g_v0"])


@pytest.mark.parametrize("mode", MODES)
def test_a_rows_bits_do_not_depend_on_the_later_batch_items(mode):
    """`exact` (B 3): the masks are functions of an item's index in the call, so the first one or two items alone give their bits of the whole batch — outputs and
    input gradients (the parameter gradients sum over the batch)."""
    c = _case("exact")
    ins = [c[k] for k in INS]
    p, seed = 0.1, 0xABCDEF0123
    full = _step("exact", mode, ins, c["g_out0"], c["g_out1"], p, seed, want_p=set())
    for nb in (1, 2):
        part = _step("exact", mode, [x[:nb] for x in ins], c["g_out0"][:nb], c["g_out1"][:nb], p, seed, want_p=set())
        assert np.array_equal(part[0], full[0][:nb]) and np.array_equal(part[1], full[1][:nb])
        assert set(part[2]) == set(stc.INPUT_GRADS) and all(np.array_equal(part[2][k], full[2][k][:nb]) for k in part[2])


def test_null_outputs_leave_the_other_bits_unchanged():
    full = _result("small", "bf16x3")
    keep = {"self_attn_layer0.linear1.weight", "cross_attn_layer0.multihead_attn.in_proj_bias", "cross_attn_layer1.norm3.weight",
            "self_attn_layer1.self_attn.out_proj.weight", "cross_attn_layer0.linear2.bias"}
    part = _full_step("small", "bf16x3", want_in=(False, True, False, False), want_p=keep)[2]
    assert set(part) == keep | {"g_pos0"}
    assert all(np.array_equal(part[k], full[k]) for k in part)
    only_inputs = _full_step("small", "bf16x3", want_p=set())[2]
    assert set(only_inputs) == set(stc.INPUT_GRADS) and all(np.array_equal(only_inputs[k], full[k]) for k in only_inputs)
    name, p, seed = _spec("small")
    c = _case(name)
    z = _step(name, "bf16x3", [c[k] for k in INS], None, None, p, seed)[2]
    assert all(not v.any() for v in z.values())


# ------------------------------------------------------------------------------------------ through the module
def _module(gid, mode="bf16x3"):
    name, p, _ = _spec(gid)
    m = base._module(_case(name), mode, dropout=p)
    m.hip_training = True
    return m.train()


def test_module_with_hip_dropout_and_a_seed_meets_the_golden():
    name, p, seed = _spec("small")
    c, ref = _case(name), _ref("small")
    m = _module("small")
    m.hip_dropout, m.dropout_seed = True, seed
    t = [_dev(c[k]).requires_grad_(True) for k in INS]
    o0, o1 = m(*t)
    ((o0 * _dev(c["g_out0"])).sum() + (o1 * _dev(c["g_out1"])).sum()).backward()
    assert m.pack_count == 1 and m._train_cache.pack_count == 1
    got = {"out0": o0.detach().cpu().numpy(), "out1": o1.detach().cpu().numpy()}
    got.update({k: x.grad.cpu().numpy() for k, x in zip(stc.INPUT_GRADS, t)})
    got.update({n: q.grad.cpu().numpy() for n, q in m.named_parameters() if q.grad is not None})
    assert set(got) == set(ref)
    errs, k = _worst(got, ref)
    print(f"sct module hip_dropout small: worst {errs[k]:.2e} ({k})")
    assert errs[k] <= BAR
    res = _result("small", "bf16x3")
    assert all(np.array_equal(got[k], res[k]) for k in got)   # the module is the library call
    m.eval()   # eval mode: no dropout, the plain step
    e0, _ = m(*[_dev(c[k]).requires_grad_(True) for k in INS])
    assert m.pack_count == 1 and np.array_equal(e0.detach().cpu().numpy(), base._lib_forward("small", "bf16x3", [c[k] for k in INS])[0])


def test_module_seeds_follow_torch_manual_seed():
    name, _, _ = _spec("small")
    c = _case(name)
    m = _module("small")
    m.hip_dropout = True
    assert m.dropout_seed is None
    run = lambda: m(*[_dev(c[k]) for k in INS])[0].detach().cpu().numpy()
    torch.manual_seed(1234)
    a, a2 = run(), run()
    torch.manual_seed(1234)
    b = run()
    assert m.pack_count == 1
    assert np.array_equal(a, b) and not np.array_equal(a, a2)   # the same seed after the same manual_seed; consecutive forwards draw new ones


def test_module_without_hip_dropout_stays_eager():
    name, _, _ = _spec("small")
    c = _case(name)
    m = _module("small")
    assert m.hip_dropout is False
    o0, _ = m(*[_dev(c[k]) for k in INS])
    assert o0.requires_grad and m.pack_count == 0 and m._train_cache.pack_count == 0
    m.hip_dropout = True
    m.dropout = 1.0   # p >= 1 stays eager
    o0, _ = m(*[_dev(c[k]) for k in INS])
    assert o0.requires_grad and m.pack_count == 0
