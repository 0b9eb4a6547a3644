"""GPU tests of the fine matcher's training step (csrc/fine_bwd.hip: nl_fine_match_backward, nl_fine_windows_backward, and nerf_loc_amd.fine_matching in training
mode): gradients against the reference's fp64 goldens and the fp64 restatement, bit reproducibility, the frozen-weights form, workspace guards, the module path."""
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess
from tests import fine_train_cases as tc
from tests import fine_train_ref as ref
from tests.test_gpu_match_train import _buf, _guards_intact

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")   # the modes held to the parity bar (bf16: throughput mode, not held)
BAR = 1e-4
DEV = "cuda:0"
WIN_NAMES = ("feat_f",) + tc.PROJ_NAMES


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_windows_bwd(c, mode, g_out, null_params=False, guard=False, null_map=False):
    """nl_fine_windows_backward on a case with the cotangent g_out (M, 49, Cout) (device tensor): {feat_f (B,Cf,Hf,Wf), proj.weight, proj.bias}, guards_ok."""
    lib = _lib.load()
    case = c["case"]
    B, Cf, Hf, Wf, Cout, M = case.B, case.Cf, case.Hf, case.Wf, case.Cout, len(c["j_ids"])
    st = torch.cuda.current_stream().cuda_stream
    w, b = _dev(c["proj"]["proj.weight"]), _dev(c["proj"]["proj.bias"])
    need = lib.nl_fine_proj_packed_bytes(Cf, Cout)
    packed = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_fine_pack_proj(Cf, Cout, w.data_ptr(), b.data_ptr(), packed.data_ptr(), need, st), "pack")
    tneed = lib.nl_fine_proj_train_bytes(Cf, Cout)
    tpacked = torch.empty(tneed, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_fine_pack_proj_train(Cf, Cout, w.data_ptr(), tpacked.data_ptr(), tneed, st), "pack_train")
    nhwc = _dev(c["feat_f"].transpose(0, 2, 3, 1))
    bi, ji = _dev(c["b_ids"]), _dev(c["j_ids"])
    g_w = None if null_params else torch.empty((Cout, Cf), dtype=torch.float32, device=DEV)
    g_b = None if null_params else torch.empty((Cout,), dtype=torch.float32, device=DEV)
    g_map = None if null_map else torch.full((B, Hf, Wf, Cf), float("nan"), dtype=torch.float32, device=DEV)   # every pixel must be written
    wneed = lib.nl_fine_windows_backward_workspace_bytes(Cf, Cout, B, Hf, Wf, case.s, M)
    whole, ws = _buf(wneed, guard)
    _lib.check(lib.nl_fine_windows_backward(packed.data_ptr(), tpacked.data_ptr(), Cf, Cout, _lib.PRECISIONS[mode], nhwc.data_ptr(), B, Hf, Wf, bi.data_ptr(),
                                            ji.data_ptr(), M, case.s, g_out.data_ptr(), _ptr(g_w), _ptr(g_b), _ptr(g_map), ws.data_ptr(), wneed, st), "windows_backward")
    torch.cuda.synchronize()
    out = {}
    if g_map is not None:
        out["feat_f"] = g_map.permute(0, 3, 1, 2).cpu().numpy()
    if not null_params:
        out.update({"proj.weight": g_w.cpu().numpy(), "proj.bias": g_b.cpu().numpy()})
    return out, (not guard) or _guards_intact(whole, wneed)


def run_lib(c, mode, null_params=False, guard=False, rows=None):
    """The chain through the C-ABI: nl_fine_windows, nl_fine_match (heat-map), nl_fine_match_backward, nl_fine_windows_backward.  rows: the window rows the match
    stage runs on instead of nl_fine_windows' (the reference's own, as tests/test_gpu_fine.py drives that stage).
    -> dict(expec_f, grads {name: numpy}, g_f1 (device), guards_ok)."""
    lib = _lib.load()
    case = c["case"]
    Cout, M = case.Cout, len(c["j_ids"])
    prec = _lib.PRECISIONS[mode]
    st = torch.cuda.current_stream().cuda_stream
    pre = FinePreprocess(tc.fc.preprocess_config(case), precision=mode)
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    if rows is None:   # the training forward's rows: FinePreprocess.train_rows_precision (exact fp32 in both parity modes)
        f1 = pre.to(DEV)._windows_call(_dev(c["feat_f"]), _dev(c["b_ids"]), _dev(c["j_ids"]), case.s, pre.train_rows_precision())[0]
    else:
        f1 = _dev(rows.astype(np.float32))
    ws_ = [_dev(c["mlp"][n]) for n in tc.MLP_NAMES]
    need = lib.nl_s2d_packed_weights_bytes(Cout)
    packed = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_s2d_pack_weights(Cout, *[t.data_ptr() for t in ws_], packed.data_ptr(), need, st), "pack")
    tneed = lib.nl_s2d_train_weights_bytes(Cout)
    tpacked = torch.empty(tneed, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_s2d_pack_train_weights(Cout, ws_[0].data_ptr(), ws_[2].data_ptr(), tpacked.data_ptr(), tneed, st), "pack_train")
    f0, kc, ge = _dev(c["feat_f0"]), _dev(c["mkps2d_c"]), _dev(c["g_expec"])
    expec = torch.empty((M, 3), dtype=torch.float32, device=DEV)
    kf = torch.empty((M, 2), dtype=torch.float32, device=DEV)
    heat = torch.empty((M, 49), dtype=torch.float32, device=DEV)
    _lib.check(lib.nl_fine_match(packed.data_ptr(), Cout, prec, f0.data_ptr(), f1.data_ptr(), M, kc.data_ptr(), expec.data_ptr(), kf.data_ptr(), heat.data_ptr(), st),
               "match")
    g_f0 = torch.full_like(f0, float("nan"))
    g_f1 = torch.full_like(f1, float("nan"))
    g_p = [None] * 6 if null_params else [torch.empty_like(t) for t in ws_]
    bneed = lib.nl_fine_match_backward_workspace_bytes(M, Cout)
    whole, ws = _buf(bneed, guard)
    _lib.check(lib.nl_fine_match_backward(packed.data_ptr(), tpacked.data_ptr(), Cout, prec, f0.data_ptr(), f1.data_ptr(), M, heat.data_ptr(), ge.data_ptr(),
                                          g_f0.data_ptr(), g_f1.data_ptr(), *[_ptr(g) for g in g_p], ws.data_ptr(), bneed, st), "match_backward")
    wg, wok = run_windows_bwd(c, mode, g_f1, null_params=null_params, guard=guard)
    torch.cuda.synchronize()
    grads = {"feat_f0": g_f0.cpu().numpy(), "feat_f1": g_f1.cpu().numpy()}
    grads.update(wg)
    if not null_params:
        grads.update({n: g.cpu().numpy() for n, g in zip(tc.MLP_NAMES, g_p)})
    return dict(expec_f=expec.cpu().numpy(), grads=grads, g_f1=g_f1, rows=f1, guards_ok=wok and ((not guard) or _guards_intact(whole, bneed)))


B3 = "mlps.4.bias"   # expec_f does not depend on it (the softmax ignores a shift of the logits): the library writes an exact zero, autograd leaves rounding noise


def _check(tag, got, want, devs, names, zero=()):
    """tests/test_gpu_match_train.py's rule: max |error| / max |reference| below max(1e-4, 3 x the reference's own fp32-vs-fp64 deviation); exact zeros where the
    reference gradient is identically zero, and for mlps.4.bias (a deviation relative to its fp64 rounding noise would be a bound that cannot fail)."""
    worst = []
    for n in names:
        if n in zero or n == B3:
            if n != B3:
                assert not np.asarray(want[n]).any(), n
            ok = not got[n].any()
            print(f"fine train {tag}: grad {n} exactly zero: {ok}")
            if not ok:
                worst.append((n, float(np.abs(got[n]).max())))
            continue
        e, bound = _rel(got[n], want[n]), max(BAR, 3 * devs.get(n, 0.0))
        print(f"fine train {tag}: grad {n} max-rel {e:.3e} (bound {bound:.1e})")
        if not e < bound:
            worst.append((n, e))
    assert not worst, worst


_REF = {}


def _case_ref(name):
    if name not in _REF:   # fp64 on the CPU: once per session, not once per mode
        c = tc.make_case(name)
        _REF[name] = (c, ref.train_step(c))
    return _REF[name]


def _golden_check(name, tag, got):
    g = tc.load_grad_golden(GOLDEN, name)
    print(f"fine train {name} {tag}: expec_f max-abs {np.abs(got['expec_f'] - g['expec_f']).max():.3e}")
    assert np.isfinite(got["grads"]["feat_f1"]).all()
    _check(f"{name} {tag}", got["grads"], {n: g["grad_" + tc.key(n)] for n in tc.GRAD_NAMES}, {n: float(g["dev_" + tc.key(n)]) for n in tc.GRAD_NAMES},
           tc.GRAD_NAMES, zero=tc.FLAT_ZERO if name == "flat" else ())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_gradients_against_the_reference_goldens(name, mode):
    """The whole chain through the C-ABI, nothing of the reference in it: nl_fine_windows (the training forward's rows) -> nl_fine_match with the heat-map ->
    nl_fine_match_backward -> nl_fine_windows_backward, every gradient against the reference's fp64 golden."""
    _golden_check(name, mode, run_lib(_case_ref(name)[0], mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_match_stage_on_the_reference_rows(name, mode):
    """In addition, per stage as tests/test_gpu_fine.py drives it: the match stage (forward with the heat-map, backward) on the rows the reference's
    FinePreprocess produced (tests/golden/fine_<case>_rows*.npz), the windows stage on its result."""
    rows = tc.fc.load_golden(GOLDEN, name)["feat_f1"]
    _golden_check(name, mode + " (reference rows)", run_lib(_case_ref(name)[0], mode, rows=rows))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_windows_stage_alone_against_the_restatement(name, mode):
    """nl_fine_windows_backward driven with the restatement's fp64 g_f1 (rounded to fp32) as cotangent, against the restatement's fp64 results."""
    c, r = _case_ref(name)
    got, _ = run_windows_bwd(c, mode, _dev(r["g_f1"].astype(np.float32)))
    _check(f"windows {name} {mode}", got, r["grads"], {}, WIN_NAMES, zero=WIN_NAMES if name == "flat" else ())
    assert np.isfinite(got["feat_f"]).all()   # every pixel written, the ones no window covers as zero
    covered = np.abs(r["grads"]["feat_f"]).sum(axis=1) > 0
    assert not got["feat_f"].transpose(0, 2, 3, 1)[~covered].any()


_LARGE = {}


@pytest.mark.parametrize("mode", MODES)
def test_gradients_at_a_shape_with_many_windows_and_matches(mode):
    """c192 at M 1100 on a 120 x 160 map (stride 4: 1200 windows per image): more windows than the scan has threads, several workgroups of the count and
    placement kernels, window lists that need more than one search step.  The whole chain against the fp64 restatement, the flat bar (no recorded deviation).

    The restatement's backward is evaluated at the rows the training forward wrote (themselves held to the fp64 rows), not at its own fp64 rows: among this
    shape's 6.9 million layer-1 units one lies so close to its kink that ANY fp32 forward of the rows puts it on the other side — torch's on the CPU does
    (rows 7.8e-7 from fp64, one unit flipped), and the restatement run on those rows moves by 2.534e-3 in feat_f and 1.535e-3 in feat_f0, the very figures the
    library shows against the fp64 rows (2.535e-3, 1.535e-3).  That is the reference's own fp32-vs-fp64 deviation at this shape, for which no fixture exists."""
    got = run_lib(_LARGE["c"], mode) if _LARGE else None
    if not _LARGE:   # fp64 on the CPU: once, not once per mode (both parity modes compute the training forward's rows in exact fp32: the same bits)
        c = tc.make_case(tc.scaled("c192", 1100, 120, 160))
        got = run_lib(c, mode)
        rows = got["rows"].cpu().numpy()
        f1_64 = ref.train_step(c)["feat_f1"]
        mb = ref.match_backward(c["feat_f0"], rows, c["mlp"], c["g_expec"])
        grads = {k: v for k, v in mb["grads"].items() if k != "feat_f1"}
        grads.update(ref.windows_backward(c["feat_f"], c["b_ids"], c["j_ids"], c["case"].s, c["proj"], mb["grads"]["feat_f1"]))
        _LARGE.update(c=c, rows=rows, f1_64=f1_64, expec_f=mb["expec_f"], grads=grads)
    assert np.array_equal(got["rows"].cpu().numpy(), _LARGE["rows"])
    e_rows = _rel(_LARGE["rows"], _LARGE["f1_64"])
    print(f"fine train large {mode}: rows max-rel {e_rows:.3e} expec_f max-abs {np.abs(got['expec_f'] - _LARGE['expec_f']).max():.3e}")
    assert e_rows < BAR
    _check(f"large {mode}", got["grads"], _LARGE["grads"], {}, tc.GRAD_NAMES)


def test_two_calls_give_the_same_bits():
    for name in ("repeat", "s1", "odd4"):
        c = _case_ref(name)[0]
        a, b = run_lib(c, "bf16x3"), run_lib(c, "bf16x3")
        assert np.array_equal(a["expec_f"], b["expec_f"])
        for n in tc.GRAD_NAMES + ("feat_f1",):
            assert np.array_equal(a["grads"][n], b["grads"][n]), (name, n)


@pytest.mark.parametrize("mode", MODES + ("bf16",))
def test_null_parameter_pointers_leave_the_feature_and_map_gradients_bit_identical(mode):
    c = _case_ref("repeat")[0]
    a, b = run_lib(c, mode), run_lib(c, mode, null_params=True)
    for n in ("feat_f0", "feat_f1", "feat_f"):
        assert np.array_equal(a["grads"][n], b["grads"][n]), n
    assert all(np.isfinite(a["grads"][n]).all() for n in tc.GRAD_NAMES)
    # the feature-gradient pointers may be NULL too
    got, _ = run_windows_bwd(c, mode, a["g_f1"], null_map=True)
    assert np.array_equal(got["proj.weight"], a["grads"]["proj.weight"]) and np.array_equal(got["proj.bias"], a["grads"]["proj.bias"])


@pytest.mark.parametrize("name", ("borders", "single", "c256"))
def test_workspace_guards_stay_intact_at_the_queried_size(name):
    c = _case_ref(name)[0]
    got = run_lib(c, "bf16x3", guard=True)
    assert got["guards_ok"]
    plain = run_lib(c, "bf16x3")
    for n in tc.GRAD_NAMES:
        assert np.array_equal(got["grads"][n], plain["grads"][n]), n


def test_no_matches_write_zeros():
    lib = _lib.load()
    g_w = torch.full((64, 64), 7.0, device=DEV)
    g_b = torch.full((64,), 7.0, device=DEV)
    g_map = torch.full((1, 4, 5, 64), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.nl_fine_windows_backward(None, None, 64, 64, _lib.PREC_BF16X3, None, 1, 4, 5, None, None, 0, 2, None, g_w.data_ptr(), g_b.data_ptr(),
                                            g_map.data_ptr(), None, 0, st), "windows_backward M = 0")
    torch.cuda.synchronize()
    assert not g_w.any() and not g_b.any() and not g_map.any()


# ------------------------------------------------------------------------------------------ through the modules
def _modules(c, loss_type="l2_with_std", hip=True, mode="bf16x3"):
    pre = FinePreprocess(tc.fc.preprocess_config(c["case"]), precision=mode)
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    fm = FineMatching(tc.fc.matching_config(c["case"], loss_type), precision=mode)
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
    pre.hip_training = fm.hip_training = hip
    return pre.to(DEV), fm.to(DEV)


def _step(pre, fm, c, train=True, nhwc_input=False):
    pre.train(train), fm.train(train)
    pre.zero_grad(set_to_none=True), fm.zero_grad(set_to_none=True)
    if nhwc_input:
        base = _dev(c["feat_f"].transpose(0, 2, 3, 1)).requires_grad_(True)
        feat_f = base.permute(0, 3, 1, 2)
    else:
        base = feat_f = _dev(c["feat_f"]).requires_grad_(True)
    feat_f0 = _dev(c["feat_f0"]).requires_grad_(True)
    data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": _dev(c["b_ids"]), "j_ids": _dev(c["j_ids"]),
            "mkps2d_c": _dev(c["mkps2d_c"]), "expec_f_gt": _dev(c["expec_f_gt"])}
    fm(feat_f0, pre(feat_f, None, data), data)
    total = data["fine_loss"] if train else (data["expec_f"] * _dev(c["g_expec"])).sum()
    total.backward()
    torch.cuda.synchronize()
    grads = {"feat_f": base.grad, "feat_f0": feat_f0.grad}
    grads.update({n: p.grad for n, p in list(pre.named_parameters()) + list(fm.named_parameters())})
    return data, {k: (None if v is None else v.detach().cpu().numpy()) for k, v in grads.items()}, base


@pytest.mark.parametrize("loss_type", tc.LOSS_TYPES)
def test_module_train_step_fills_every_gradient_like_the_eager_path(loss_type):
    c = _case_ref(tc.TRAIN_CASE)[0]
    g = tc.load_grad_golden(GOLDEN, tc.TRAIN_CASE)
    data, got, _ = _step(*_modules(c, loss_type), c)
    edata, want, _ = _step(*_modules(c, loss_type, hip=False), c)
    assert data["fine_loss"].requires_grad and data["expec_f"].requires_grad and not data["mkps2d_f"].requires_grad
    assert "FineMatchFn" in type(data["expec_f"].grad_fn).__name__   # one Function, not the eager graph
    el = abs(float(data["fine_loss"].detach()) - float(edata["fine_loss"].detach())) / abs(float(edata["fine_loss"].detach()))
    print(f"fine module {loss_type}: loss rel vs eager {el:.3e}, vs golden {abs(float(data['fine_loss'].detach()) - float(g['loss_' + loss_type])) / abs(float(g['loss_' + loss_type])):.3e}")
    assert el <= BAR
    names = tuple(n for n in tc.GRAD_NAMES if n != "mlps.4.bias")
    for n in tc.GRAD_NAMES:
        assert got[n] is not None and want[n] is not None, n
    # against the reference's fp64 gradients of the loss, the project's bar; and against the eager path
    _check(f"module {loss_type}", got, {n: g[f"lossgrad_{loss_type}_{tc.key(n)}"] for n in tc.GRAD_NAMES},
           {n: float(g[f"lossdev_{loss_type}_{tc.key(n)}"]) for n in tc.GRAD_NAMES}, tc.GRAD_NAMES)
    for n in names:
        e = _rel(got[n], want[n].astype(np.float64))
        print(f"fine module {loss_type}: grad {n} vs eager max-rel {e:.3e}")
        assert e < BAR, n
    # mlps.4.bias: the softmax ignores a shift of the logits, so this gradient is rounding noise around zero under autograd and an exact zero in the library
    scale = float(np.abs(got["mlps.4.weight"]).max())
    assert float(got["mlps.4.bias"][0]) == 0.0 and abs(float(want["mlps.4.bias"][0])) <= 1e-4 * scale


def test_module_eval_mode_differentiates_the_inputs_and_leaves_the_parameters_alone():
    c, r = _case_ref("odd4")
    data, got, _ = _step(*_modules(c), c, train=False)
    assert "fine_loss" not in data
    for n in tc.PROJ_NAMES + tc.MLP_NAMES:
        assert got[n] is None, n   # NULL parameter-gradient pointers: no weight-gradient work, no .grad
    _check("module eval", got, r["grads"], {}, ("feat_f", "feat_f0"))


def test_module_frozen_parameters_get_no_gradient_and_double_backward_raises():
    c = _case_ref(tc.TRAIN_CASE)[0]
    pre, fm = _modules(c)
    pre.proj.weight.requires_grad_(False)
    fm.mlps[0].weight.requires_grad_(False)
    fm.mlps[4].bias.requires_grad_(False)
    _, got, _ = _step(pre, fm, c)
    assert got["proj.weight"] is None and got["mlps.0.weight"] is None and got["mlps.4.bias"] is None
    assert got["proj.bias"] is not None and got["mlps.2.weight"] is not None and got["feat_f"] is not None and got["feat_f0"] is not None
    pre2, fm2 = _modules(c)
    pre2.train(), fm2.train()
    feat_f0 = _dev(c["feat_f0"]).requires_grad_(True)
    data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": _dev(c["b_ids"]), "j_ids": _dev(c["j_ids"]),
            "mkps2d_c": _dev(c["mkps2d_c"]), "expec_f_gt": _dev(c["expec_f_gt"])}
    fm2(feat_f0, pre2(_dev(c["feat_f"]), None, data), data)
    (gg,) = torch.autograd.grad(data["fine_loss"], feat_f0, create_graph=True)
    with pytest.raises(RuntimeError):
        gg.sum().backward()


def test_module_training_images_are_cached_and_repacked_on_change():
    c = _case_ref(tc.TRAIN_CASE)[0]
    pre, fm = _modules(c)
    _step(pre, fm, c)
    _step(pre, fm, c)
    assert pre._train_cache.pack_count == 1 and fm._train_cache.pack_count == 1 and pre.pack_count == 1 and fm.pack_count == 1
    with torch.no_grad():
        fm.mlps[2].weight.mul_(1.5)
        pre.proj.weight.mul_(0.5)
    _, got, _ = _step(pre, fm, c, train=False)
    assert pre._train_cache.pack_count == 2 and fm._train_cache.pack_count == 2
    c2 = dict(c)
    c2["mlp"] = {**c["mlp"], "mlps.2.weight": c["mlp"]["mlps.2.weight"] * np.float32(1.5)}
    c2["proj"] = {**c["proj"], "proj.weight": c["proj"]["proj.weight"] * np.float32(0.5)}
    r = ref.train_step(c2)
    assert _rel(got["feat_f"], r["grads"]["feat_f"]) < BAR and _rel(got["feat_f0"], r["grads"]["feat_f0"]) < BAR


def test_module_takes_the_eager_path_above_the_backward_limit(monkeypatch):
    """The choice is made at forward time: more matches than the backward calls accept (NL_FINE_BACKWARD_MAX_M) train on the eager path, nothing raises in backward()."""
    c = _case_ref(tc.TRAIN_CASE)[0]
    monkeypatch.setattr(_lib, "FINE_BACKWARD_MAX_M", len(c["j_ids"]) - 1)
    data, got, _ = _step(*_modules(c), c)
    assert "FineMatchFn" not in type(data["expec_f"].grad_fn).__name__
    assert all(got[n] is not None for n in tc.GRAD_NAMES)
    monkeypatch.setattr(_lib, "FINE_BACKWARD_MAX_M", len(c["j_ids"]))
    data, _, _ = _step(*_modules(c), c)
    assert "FineMatchFn" in type(data["expec_f"].grad_fn).__name__


def test_module_nhwc_map_receives_its_gradient_without_a_layout_copy():
    c, r = _case_ref("repeat")
    _, got, base = _step(*_modules(c), c, train=False, nhwc_input=True)
    assert base.grad is not None and base.grad.shape == base.shape and base.grad.is_contiguous()   # the NHWC leaf's gradient is NHWC-contiguous as the library wrote it
    assert _rel(got["feat_f"].transpose(0, 3, 1, 2), r["grads"]["feat_f"]) < BAR
