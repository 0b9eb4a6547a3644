"""GPU tests of the SelfCrossTransformer training step (csrc/sct_bwd.hip through nl_sct_forward_train / nl_sct_backward / nl_sct_layer_backward and the module's
hip_training path): forward bits, every gradient against the reference's goldens (C = 64) or the fp64 restatement (C >= 128), each layer on its own, key / query
tails, determinism, batch invariance, NULL outputs, the module, and the chain into FineMatching under one backward().
The bar of the parity modes: per tensor, max |error| <= 1e-4 x max |reference|."""
import ctypes
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_train_cases as stc
from tests import sct_train_ref as str_

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")
BAR = 1e-4
DEV = "cuda:0"
INS = ("v0", "pos0", "v1", "pos1")

_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = stc.make_case(name)
    return _CACHE[name]


def _ref(name):
    """The reference gradients of a case, {tensor name: fp64-accurate array} (computed or loaded once, never modified): the reference's goldens for the C = 64
    recipes, the fp64 restatement for the others."""
    key = ("ref", name)
    if key not in _CACHE:
        if name in stc.GOLDEN_CASES:
            g = stc.load_grad_golden(GOLDEN, name)
            r = {k: g[k] for k in stc.INPUT_GRADS}
            r.update({n: g[stc.key(n)] for n in stc.PARAM_NAMES})
        else:
            full = str_.grads(_case(name))
            r = {k: full[k] for k in stc.INPUT_GRADS + stc.PARAM_NAMES}
        _CACHE[key] = r
    return _CACHE[key]


def _module(c, mode="bf16x3", **kw):
    from nerf_loc_amd.transformer import SelfCrossTransformer
    case = c["case"]
    m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, precision=mode, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    return m.to(DEV).eval()


def _images(name):
    key = ("images", name)
    if key not in _CACHE:
        m = _module(_case(name))
        _CACHE[key] = (m, m._pack(torch.device(DEV)), m._pack_train(torch.device(DEV)))
    return _CACHE[key][1:]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _step(name, mode, ins, g0, g1, want_in=(True,) * 4, want_p=None, backward=True):
    """nl_sct_forward_train (+ nl_sct_backward) on numpy inputs: (out0, out1, {name: gradient as numpy}); want_in / want_p (a set of state names; None: all)
    choose the outputs that are not NULL."""
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
    _lib.check(lib.nl_sct_forward_train(packed.data_ptr(), C, sc.NHEAD, F, prec, t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(), t[3].data_ptr(), N1, B,
                                        o0.data_ptr(), o1.data_ptr(), state.data_ptr(), sb, ws.data_ptr(), wb, st), "nl_sct_forward_train")
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
        _lib.check(lib.nl_sct_backward(packed.data_ptr(), tpacked.data_ptr(), C, sc.NHEAD, F, prec, t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(),
                                       t[3].data_ptr(), N1, B, state.data_ptr(), sb, _ptr(tg0), _ptr(tg1), _ptr(gin[0]), _ptr(gin[1]), _ptr(gin[2]), _ptr(gin[3]),
                                       arr, 52, bws.data_ptr(), bb, st), "nl_sct_backward")
        torch.cuda.synchronize()
        grads = {k: g.cpu().numpy() for k, g in zip(stc.INPUT_GRADS, gin) if g is not None}
        grads.update({n: g.cpu().numpy() for n, g in zip(sc.STATE_NAMES, gpar) if g is not None})
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy(), grads


def _full_step(name, mode, **kw):
    c = _case(name)
    return _step(name, mode, [c[k] for k in INS], c["g_out0"], c["g_out1"], **kw)


def _rel(a, ref):
    assert np.isfinite(a).all()
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    err = np.abs(a.astype(np.float64) - ref).max()
    if scale == 0:   # an identically zero reference (`one`: the position encodings): 1e-4 x 0 admits exact zeros only
        return 0.0 if err == 0 else float("inf")
    return float(err / scale)


def _worst(grads, ref):
    errs = {k: _rel(grads[k], ref[k]) for k in ref}
    k = max(errs, key=errs.get)
    return errs, k


def _lib_forward(name, mode, ins):
    case = sc.CASES[name]
    lib = _lib.load()
    t = [_dev(a) for a in ins]
    B, N0, N1 = t[0].shape[0], t[0].shape[1], t[2].shape[1]
    o0 = torch.empty((B, N0, case.C), dtype=torch.float32, device=DEV)
    o1 = torch.empty((B, N1, case.C), dtype=torch.float32, device=DEV)
    need = lib.nl_sct_workspace_bytes(B, N0, N1, case.C, case.F)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_sct_forward(_images(name)[0].data_ptr(), case.C, sc.NHEAD, case.F, _lib.PRECISIONS[mode], t[0].data_ptr(), t[1].data_ptr(), N0, t[2].data_ptr(),
                                  t[3].data_ptr(), N1, B, o0.data_ptr(), o1.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "nl_sct_forward")
    torch.cuda.synchronize()
    return o0.cpu().numpy(), o1.cpu().numpy()


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", MODES + ("bf16",))
@pytest.mark.parametrize("name", tuple(sc.CASES))
def test_training_forward_has_the_inference_forwards_bits(name, mode):
    c = _case(name)
    ins = [c[k] for k in INS]
    a0, a1 = _lib_forward(name, mode, ins)
    b0, b1, _ = _step(name, mode, ins, None, None, backward=False)
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)


# ------------------------------------------------------------------------------------------ gradients against the reference
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", stc.GOLDEN_CASES + stc.REF_CASES)
def test_gradients_against_the_reference(name, mode):
    ref = _ref(name)
    assert len(ref) == 4 + 48
    _, _, grads = _full_step(name, mode)
    assert set(grads) == set(ref)
    errs, k = _worst(grads, ref)
    src = "golden" if name in stc.GOLDEN_CASES else "fp64 restatement"
    print(f"sct backward {name} {mode} vs {src}: worst max |error| / max |reference| {errs[k]:.2e} ({k}); inputs " +
          " ".join(f"{n} {errs[n]:.2e}" for n in stc.INPUT_GRADS))
    bad = {n: e for n, e in errs.items() if e > BAR}
    assert not bad, bad


def test_one_key_gives_exact_zero_position_gradients():
    """`one` (N0 = N1 = 1): a one-key softmax ignores q and k, so the position encodings get no gradient at all."""
    _, _, grads = _full_step("one", "bf16x3")
    assert not grads["g_pos0"].any() and not grads["g_pos1"].any()


def test_throughput_mode_runs():
    ref = _ref("small")
    _, _, grads = _full_step("small", "bf16")
    errs, k = _worst(grads, ref)
    print(f"sct backward small bf16 (not held to the bar): worst {errs[k]:.2e} ({k})")
    assert all(np.isfinite(g).all() for g in grads.values())


# ------------------------------------------------------------------------------------------ one layer at a time
def _layer_backward(name, mode, l, x, px, mem, pm, g_out):
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
    _lib.check(lib.nl_sct_layer_backward(packed.data_ptr(), tpacked.data_ptr(), C, sc.NHEAD, F, l, _lib.PRECISIONS[mode], tx.data_ptr(), tpx.data_ptr(), Nq, _ptr(tm),
                                         _ptr(tpm), Nk, B, tg.data_ptr(), gx.data_ptr(), gpx.data_ptr(), _ptr(gm), _ptr(gpm), arr, len(names), ws.data_ptr(), bb,
                                         torch.cuda.current_stream().cuda_stream), "nl_sct_layer_backward")
    torch.cuda.synchronize()
    res = {"g_x": gx.cpu().numpy(), "g_pos_x": gpx.cpu().numpy()}
    if cross:
        res.update({"g_mem": gm.cpu().numpy(), "g_pos_mem": gpm.cpu().numpy()})
    res.update({n: g.cpu().numpy() for n, g in zip(names, gpar) if g is not None})
    return res


def _outs(name):
    key = ("outs", name)
    if key not in _CACHE:
        from tests import sct_ref as sr
        _CACHE[key] = sr.forward(_case(name), torch.float64)
    return _CACHE[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("c192", "fine", "peaked"))
def test_each_layer_against_fp64_autograd(name, mode):
    from tests import sct_ref as sr
    c, outs = _case(name), _outs(name)
    worst = []
    for l in range(4):
        x, px, mem, pm = sr.layer_inputs(c, outs, l)   # the restatement's own intermediates: an error belongs to its layer
        g_out = c["g_out0"] if l in (0, 2) else c["g_out1"]
        ref = {k: v for k, v in str_.layer_grads(c, l, x, px, mem, pm, g_out).items() if v is not None}
        got = _layer_backward(name, mode, l, x, px, mem, pm, g_out)
        assert set(got) == set(ref)
        errs, k = _worst(got, ref)
        worst.append((errs[k], k))
        assert errs[k] <= BAR, (l, k, errs[k])
    print(f"sct layer backward {name} {mode}: " + " ".join(f"layer {l} {e:.2e} ({k.split('.', 1)[-1]})" for l, (e, k) in enumerate(worst)))


@pytest.mark.parametrize("mode", MODES)
def test_key_and_query_tails(mode):
    from tests import sct_ref as sr
    c, outs = _case("long"), _outs("long")
    x, px, mem, pm = sr.layer_inputs(c, outs, 2)
    w = "cross_attn_layer0.multihead_attn.in_proj_weight"
    worst = (0.0, None)
    for nq in (1, 33, 130):
        for nk in (1, 31, 32, 33, 64, 65, 129, 1100):
            a = (x[:, :nq], px[:, :nq], mem[:, :nk], pm[:, :nk])
            g_out = c["g_out0"][:, :nq]
            ref = str_.layer_grads(c, 2, *a, g_out)
            got = _layer_backward("long", mode, 2, *a, g_out)
            for k in ("g_x", "g_pos_x", "g_mem", "g_pos_mem", w):
                e = _rel(got[k], ref[k])
                worst = max(worst, (e, (nq, nk, k)))
                assert e <= BAR, (nq, nk, k, e)
    print(f"sct backward tails {mode}: worst max |error| / max |reference| over 24 (Nq, Nk) cuts {worst[0]:.2e} at {worst[1]}")


# ------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("mode", MODES + ("bf16",))
def test_backward_twice_gives_the_same_bits(mode):
    a, b = _full_step("c128", mode)[2], _full_step("c128", mode)[2]
    assert set(a) == set(b) and len(a) == 52
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_permutation_permutes_the_input_gradients(mode):
    c = _case("fine64")
    perm = np.arange(c["case"].B)[::-1].copy()
    ins = [c[k] for k in INS]
    a = _step("fine64", mode, ins, c["g_out0"], c["g_out1"], want_p=set())[2]
    b = _step("fine64", mode, [x[perm] for x in ins], c["g_out0"][perm], c["g_out1"][perm], want_p=set())[2]
    assert set(a) == set(stc.INPUT_GRADS)
    assert all(np.array_equal(a[k], b[k][perm]) for k in a)   # perm is its own inverse


def test_null_outputs_leave_the_other_bits_unchanged():
    full = _full_step("small", "bf16x3")[2]
    keep = {"self_attn_layer0.linear1.weight", "cross_attn_layer0.multihead_attn.in_proj_bias", "cross_attn_layer1.norm3.weight"}
    part = _full_step("small", "bf16x3", want_in=(False, True, False, False), want_p=keep)[2]
    assert set(part) == keep | {"g_pos0"}
    assert all(np.array_equal(part[k], full[k]) for k in part)
    only_inputs = _full_step("small", "bf16x3", want_p=set())[2]
    assert set(only_inputs) == set(stc.INPUT_GRADS) and all(np.array_equal(only_inputs[k], full[k]) for k in only_inputs)


def test_a_null_cotangent_is_a_zero_cotangent():
    c = _case("small")
    ins = [c[k] for k in INS]
    a = _step("small", "bf16x3", ins, c["g_out0"], None)[2]
    b = _step("small", "bf16x3", ins, c["g_out0"], np.zeros_like(c["g_out1"]))[2]
    assert all(np.array_equal(a[k], b[k]) for k in b)
    z = _step("small", "bf16x3", ins, None, None)[2]
    assert all(not v.any() for v in z.values())


# ------------------------------------------------------------------------------------------ through the module
def _module_grads(m, c, inputs_need_grad=True):
    t = [_dev(c[k]).requires_grad_(inputs_need_grad) for k in INS]
    o0, o1 = m(*t)
    ((o0 * _dev(c["g_out0"])).sum() + (o1 * _dev(c["g_out1"])).sum()).backward()
    got = {k: x.grad.cpu().numpy() for k, x in zip(stc.INPUT_GRADS, t) if x.grad is not None}
    got.update({n: p.grad.cpu().numpy() for n, p in m.named_parameters() if p.grad is not None})
    return got


@pytest.mark.parametrize("train", (False, True))
def test_module_with_hip_training(train):
    c, ref = _case("small"), _ref("small")
    m = _module(c, dropout=0.0)
    m.hip_training = True
    m.train(train)
    frozen = "cross_attn_layer0.linear2.weight"
    m.get_parameter(frozen).requires_grad_(False)
    got = _module_grads(m, c)
    assert m.pack_count == 1 and m._train_cache.pack_count == 1
    assert set(got) == set(ref) - {frozen}   # norm1.* of the cross layers keep .grad None, and so does the frozen parameter
    errs, k = _worst(got, {n: v for n, v in ref.items() if n != frozen})
    print(f"sct module hip_training small ({'train' if train else 'eval'} mode): worst {errs[k]:.2e} ({k})")
    assert errs[k] <= BAR
    with torch.no_grad():
        m.self_attn_layer1.linear1.bias.add_(0.25)   # in place: the same storage, a new version
    m.zero_grad()
    _module_grads(m, c)
    assert m.pack_count == 2 and m._train_cache.pack_count == 2


def test_module_with_dropout_in_training_mode_stays_eager():
    c = _case("small")
    m = _module(c, dropout=0.1)
    m.hip_training = True
    m.train()
    o0, _ = m(*[_dev(c[k]) for k in INS])
    assert o0.requires_grad and m.pack_count == 0 and m._train_cache.pack_count == 0
    m.eval()   # no dropout in effect: the library
    got = _module_grads(m, c)
    assert m.pack_count == 1 and _worst(got, _ref("small"))[0]["g_v0"] <= BAR


# ------------------------------------------------------------------------------------------ chain into the fine matcher
def test_chain_into_fine_matching_under_one_backward():
    from nerf_loc_amd.fine_matching import FineMatching
    from tests import fine_cases as fc
    c = _case("fine")
    fcase = fc.make_case("c192")
    M = c["case"].B
    g_expec = np.random.default_rng(7).standard_normal((M, 3)).astype(np.float32)
    g_expec[:, 2] = 0   # the std column carries no gradient in a training step (both losses detach it)

    def run(m, fm, dtype, dev):
        t = [torch.from_numpy(c[k]).to(device=dev, dtype=dtype) for k in INS]
        t[2].requires_grad_(True)
        o0, o1 = m(*t)
        data = {"mkps2d_c": torch.zeros((M, 2), dtype=dtype, device=dev), "stride_fine": 2}
        expec = fm(o0[:, 0], o1, data)["expec_f"]   # eval mode with features that require grad: the matcher's own training step (hip_training) or eager
        (expec * torch.from_numpy(g_expec).to(device=dev, dtype=dtype)).sum().backward()
        return t[2].grad.detach().cpu().numpy()

    def matcher(hip):
        fm = FineMatching(fc.matching_config(fcase["case"]), precision="bf16x3")
        fm.load_state_dict({k: torch.from_numpy(v) for k, v in fcase["mlp"].items()}, strict=True)
        fm.hip_training = hip
        return fm

    m = _module(c)
    m.hip_training = True
    ours = run(m, matcher(True).to(DEV).eval(), torch.float32, DEV)
    assert m._train_cache.pack_count == 1
    from nerf_loc_amd.transformer import SelfCrossTransformer
    r = SelfCrossTransformer(d_model=c["case"].C, nhead=sc.NHEAD, dim_feedforward=c["case"].F)
    r.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    ref = run(r.double().eval(), matcher(False).double().eval(), torch.float64, "cpu")   # the eager transformer and matcher in fp64
    e = _rel(ours, ref)
    print(f"sct -> FineMatching chain, gradient at v1: max |error| / max |reference| {e:.2e}")
    assert e <= BAR
