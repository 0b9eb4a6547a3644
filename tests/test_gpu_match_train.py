"""GPU tests of the coarse matcher's training step (csrc/s2d.hip: nl_s2d_forward_train, csrc/s2d_bwd.hip: nl_s2d_backward_train, and
nerf_loc_amd.matching.S2DMatching in training mode): loss and gradients against the reference's fp64 goldens and against the fp64 restatement, bit
reproducibility, the frozen-weights form, workspace guards, the module path and its peak memory."""
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from nerf_loc_amd.matching import S2DMatching
from tests import match_train_cases as tc
from tests import match_train_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("fp32", "bf16x3")   # the modes held to the parity bar (bf16: throughput mode, not held)
BAR = 1e-4
DEV = "cuda:0"
GUARD = 4096


def _key(n):
    return n.replace(".", "_")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _buf(nbytes, guard):
    """nbytes of device memory with GUARD bytes of 0xA5 on either side when guard is set: (whole, view)"""
    if not guard:
        t = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        return t, t
    pad = (nbytes + 255) // 256 * 256
    whole = torch.full((pad + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + nbytes:] == 0xA5).all())


def run_lib(c, mode, null_params=False, guard=False):
    """One forward + backward through the C-ABI: dict(loss, logits, scores, match_j, grads {name: numpy}, guards_ok, ws_bytes)."""
    lib = _lib.load()
    case = c["case"]
    N, M, C = case.N, case.M, case.C
    prec = _lib.PRECISIONS[mode]
    import ctypes as ct
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    ws_ = [dev(c["weights"][n]) for n in tc.mc.PARAM_NAMES]
    need = lib.nl_s2d_packed_weights_bytes(C)
    packed = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_s2d_pack_weights(C, *[t.data_ptr() for t in ws_], packed.data_ptr(), need, st), "pack")
    tneed = lib.nl_s2d_train_weights_bytes(C)
    tpacked = torch.empty(tneed, dtype=torch.uint8, device=DEV)
    _lib.check(lib.nl_s2d_pack_train_weights(C, ws_[0].data_ptr(), ws_[2].data_ptr(), tpacked.data_ptr(), tneed, st), "pack_train")
    d0, d1, tgt = dev(c["desc0"]), dev(c["desc1"]), dev(c["conf_matrix_gt"])
    scores = torch.empty((N, M), dtype=torch.float32, device=DEV)
    logits = torch.empty((N, M), dtype=torch.float32, device=DEV)
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    mj = torch.empty(N, dtype=torch.int32, device=DEV)
    ms = torch.empty(N, dtype=torch.float32, device=DEV)
    fneed = lib.nl_s2d_forward_train_workspace_bytes(N, M, C)
    fwhole, fws = _buf(fneed, guard)
    _lib.check(lib.nl_s2d_forward_train(packed.data_ptr(), C, prec, d0.data_ptr(), N, d1.data_ptr(), M, ct.c_float(c["thr"]), tgt.data_ptr(), scores.data_ptr(),
                                        logits.data_ptr(), loss.data_ptr(), mj.data_ptr(), ms.data_ptr(), fws.data_ptr(), fneed, st), "forward_train")
    gl = torch.full((1,), c["g_loss"], dtype=torch.float32, device=DEV)
    gs = None if c["g_score"] is None else dev(c["g_score"])
    g_d0, g_d1 = torch.empty_like(d0), torch.empty_like(d1)
    g_p = [None] * 6 if null_params else [torch.empty_like(t) for t in ws_]
    bneed = lib.nl_s2d_backward_train_workspace_bytes(N, M, C)
    bwhole, bws = _buf(bneed, guard)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.nl_s2d_backward_train(packed.data_ptr(), tpacked.data_ptr(), C, prec, d0.data_ptr(), N, d1.data_ptr(), M, logits.data_ptr(), tgt.data_ptr(),
                                         gl.data_ptr(), ptr(gs), g_d0.data_ptr(), g_d1.data_ptr(), *[ptr(g) for g in g_p], bws.data_ptr(), bneed, st), "backward_train")
    torch.cuda.synchronize()
    grads = {"desc0": g_d0.cpu().numpy(), "desc1": g_d1.cpu().numpy()}
    if not null_params:
        grads.update({n: g.cpu().numpy() for n, g in zip(tc.mc.PARAM_NAMES, g_p)})
    ok = (not guard) or (_guards_intact(fwhole, fneed) and _guards_intact(bwhole, bneed))
    return dict(loss=float(loss.item()), logits=logits.cpu().numpy(), scores=scores.cpu().numpy(), match_j=mj.cpu().numpy(), grads=grads, guards_ok=ok, ws_bytes=bneed)


_MID = {}


def _mid_ref():
    if not _MID:   # fp64 on the CPU: once per session, not once per mode
        c = tc.make_case("mid")
        args = (c["desc0"], c["desc1"], c["weights"], c["conf_matrix_gt"], c["g_loss"], c["g_score"])
        _MID.update(c=c, r=ref.train_step(*args, chunk=32))
    return _MID["c"], _MID["r"]


def _check(tag, got, want_loss, want_grads, devs):
    el = abs(got["loss"] - want_loss) / abs(want_loss)
    print(f"s2d train {tag}: loss rel {el:.3e}")
    worst = []
    for n in tc.GRAD_NAMES:
        e, bound = _rel(got["grads"][n], want_grads[n]), max(BAR, 3 * devs.get(n, 0.0))
        print(f"s2d train {tag}: grad {n} max-rel {e:.3e} (bound {bound:.1e})")
        if not e < bound:
            worst.append((n, e))
    assert el <= BAR
    assert not worst, worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_loss_and_gradients_against_the_reference_goldens(name, mode):
    c = tc.make_case(name)
    g = np.load(os.path.join(GOLDEN, f"s2d_grad_{name}.npz"))
    got = run_lib(c, mode)
    print(f"s2d train {name} {mode}: logits max-rel {_rel(got['logits'], g['logits']):.3e}")
    _check(f"{name} {mode}", got, float(g["loss"]), {n: g["grad_" + _key(n)] for n in tc.GRAD_NAMES}, {n: float(g["dev_" + _key(n)]) for n in tc.GRAD_NAMES})


@pytest.mark.parametrize("mode", MODES)
def test_loss_and_gradients_against_fp64_at_the_larger_shape(mode):
    """(256, 1200, 192), ten row chunks of the backward pass, a random g_score, against tests/match_train_ref.py in fp64."""
    c, r = _mid_ref()
    got = run_lib(c, mode)
    _check(f"mid {mode}", got, r["loss"], r["grads"], {})   # no recorded deviation: the flat bar


def test_two_calls_give_the_same_bits():
    for name in ("gscore", "mid"):
        c = tc.make_case(name) if name != "mid" else _mid_ref()[0]
        a, b = run_lib(c, "bf16x3"), run_lib(c, "bf16x3")
        assert a["loss"] == b["loss"] and np.array_equal(a["logits"], b["logits"])
        for n in tc.GRAD_NAMES:
            assert np.array_equal(a["grads"][n], b["grads"][n]), (name, n)


@pytest.mark.parametrize("mode", MODES + ("bf16",))
def test_null_parameter_pointers_give_the_same_descriptor_gradients(mode):
    c = tc.make_case("ragged")
    a, b = run_lib(c, mode), run_lib(c, mode, null_params=True)
    assert np.array_equal(a["grads"]["desc0"], b["grads"]["desc0"]) and np.array_equal(a["grads"]["desc1"], b["grads"]["desc1"])
    assert np.isfinite(a["grads"]["mlps.0.weight"]).all()


def test_forward_train_is_the_match_call_plus_logits():
    c = tc.make_case("small")
    got = run_lib(c, "bf16x3")
    m = S2DMatching(c["case"].C, thr=c["thr"]).to(DEV).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    s, mj, _ = m.match(torch.from_numpy(c["desc0"]).to(DEV), torch.from_numpy(c["desc1"]).to(DEV))
    assert np.array_equal(s.cpu().numpy(), got["scores"]) and np.array_equal(mj.cpu().numpy(), got["match_j"])
    assert np.array_equal(torch.sigmoid(torch.from_numpy(got["logits"])).numpy() > 0.5, got["scores"] > 0.5)


@pytest.mark.parametrize("name", ("ragged", "one", "c256"))
def test_workspace_guards_stay_intact_at_the_queried_size(name):
    c = tc.make_case(name)
    got = run_lib(c, "bf16x3", guard=True)
    assert got["guards_ok"]
    plain = run_lib(c, "bf16x3")
    for n in tc.GRAD_NAMES:
        assert np.array_equal(got["grads"][n], plain["grads"][n]), n


# ------------------------------------------------------------------------------------------ through the module
def _module(c, mode="bf16x3", hip=True):
    m = S2DMatching(c["case"].C, thr=c["thr"], precision=mode)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    m.hip_training = hip
    return m.to(DEV)


def _step(m, c, train=True, score_sum=False):
    m.train(train)
    m.zero_grad(set_to_none=True)
    d0 = torch.from_numpy(c["desc0"]).to(DEV).requires_grad_(True)
    d1 = torch.from_numpy(c["desc1"]).to(DEV).requires_grad_(True)
    data = m(d0, d1, {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"]).to(DEV)})
    total = data["score_matrix"].sum() if score_sum else data["coarse_loss"]
    total.backward()
    torch.cuda.synchronize()
    grads = {"desc0": d0.grad, "desc1": d1.grad}
    grads.update({n: p.grad for n, p in m.named_parameters()})
    return data, {k: (None if v is None else v.cpu().numpy()) for k, v in grads.items()}


def test_module_backward_fills_every_gradient_like_the_eager_path():
    c = tc.make_case("small")
    data, got = _step(_module(c), c)
    edata, want = _step(_module(c, hip=False), c)
    assert data["coarse_loss"].requires_grad and data["score_matrix"].requires_grad
    el = abs(float(data["coarse_loss"].detach()) - float(edata["coarse_loss"].detach())) / abs(float(edata["coarse_loss"].detach()))
    print(f"s2d module: loss rel {el:.3e}")
    assert el <= BAR
    for n in tc.GRAD_NAMES:
        e = _rel(got[n], want[n].astype(np.float64))
        print(f"s2d module: grad {n} vs eager max-rel {e:.3e}")
        assert e < BAR, n
    assert np.array_equal(data["i_ids"].cpu().numpy(), edata["i_ids"].cpu().numpy()) and np.array_equal(data["j_ids"].cpu().numpy(), edata["j_ids"].cpu().numpy())


def test_module_eval_mode_differentiates_the_scores_and_leaves_the_parameters_alone():
    c = tc.make_case("ragged")
    data, got = _step(_module(c), c, train=False, score_sum=True)
    edata, want = _step(_module(c, hip=False), c, train=False, score_sum=True)
    assert "coarse_loss" not in data
    for n in tc.mc.PARAM_NAMES:
        assert got[n] is None, n   # NULL parameter-gradient pointers: no weight-gradient work, no .grad
    for n in ("desc0", "desc1"):
        e = _rel(got[n], want[n].astype(np.float64))
        print(f"s2d module eval: grad {n} vs eager max-rel {e:.3e}")
        assert e < BAR, n


def test_module_frozen_parameters_get_no_gradient_and_double_backward_raises():
    c = tc.make_case("ragged")
    m = _module(c)
    m.mlps[0].weight.requires_grad_(False)
    m.mlps[4].bias.requires_grad_(False)
    _, got = _step(m, c)
    assert got["mlps.0.weight"] is None and got["mlps.4.bias"] is None and got["mlps.2.weight"] is not None and got["desc0"] is not None
    m2 = _module(c).train()
    d0 = torch.from_numpy(c["desc0"]).to(DEV).requires_grad_(True)
    data = m2(d0, torch.from_numpy(c["desc1"]).to(DEV), {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"]).to(DEV)})
    (g,) = torch.autograd.grad(data["coarse_loss"], d0, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_module_training_image_is_cached_and_repacked_on_change():
    c = tc.make_case("one")
    m = _module(c)
    _step(m, c)
    _step(m, c)
    assert m._train_cache.pack_count == 1
    with torch.no_grad():
        m.mlps[2].weight.mul_(1.5)
    _, got = _step(m, c)
    assert m._train_cache.pack_count == 2
    w = {k: v.copy() for k, v in c["weights"].items()}
    w["mlps.2.weight"] = w["mlps.2.weight"] * np.float32(1.5)
    r = ref.train_step(c["desc0"], c["desc1"], w, c["conf_matrix_gt"])
    assert _rel(got["desc0"], r["grads"]["desc0"]) < BAR


def test_module_peak_memory_stays_below_the_product_tensor():
    """(256, 1200, 192): forward + backward through the module peaks below N * M * C * 4 bytes above the starting level; the eager path needs more than twice that."""
    c, _ = _mid_ref()
    N, M, C = c["case"].N, c["case"].M, c["case"].C
    product = N * M * C * 4

    def peak(hip):
        m = _module(c, hip=hip)
        _step(m, c)   # warm-up: packed images, library load
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        _step(m, c)
        return torch.cuda.max_memory_allocated() - start
    lib_peak, eager_peak = peak(True), peak(False)
    print(f"s2d train memory (256, 1200, 192): library peak {lib_peak / 2**20:.1f} MiB, eager peak {eager_peak / 2**20:.1f} MiB, product tensor {product / 2**20:.1f} MiB")
    assert lib_peak < product
    assert eager_peak > 2 * product
