"""CPU-side checks of the coarse matcher's training step (nerf_loc_amd/matching.py, csrc/s2d_bwd.hip): the fp64 restatement tests/match_train_ref.py reproduces
the goldens the reference itself produced, the module's eager training path matches them at the parity bar, and the new entry points refuse bad arguments
before anything is dereferenced."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from nerf_loc_amd.matching import S2DMatching

from . import match_train_cases as tc
from . import match_train_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4


def golden(name):
    return np.load(os.path.join(GOLDEN, f"s2d_grad_{name}.npz"))


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-300))


def key(name):
    return name.replace(".", "_")


@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_goldens(name):
    c, g = tc.make_case(name), golden(name)
    r = ref.train_step(c["desc0"], c["desc1"], c["weights"], c["conf_matrix_gt"], c["g_loss"], c["g_score"])
    assert abs(r["loss"] - float(g["loss"])) <= 1e-9 * abs(float(g["loss"]))
    assert rel(r["logits"], g["logits"]) <= 1e-9
    for n in tc.GRAD_NAMES:
        assert rel(r["grads"][n], g["grad_" + key(n)]) <= 1e-9, n


def test_goldens_record_a_reference_deviation_within_the_generator_bar():
    for name in tc.GOLDEN_CASES:
        g = golden(name)
        for n in ("loss", "logits") + tc.GRAD_NAMES:
            assert 0.0 <= float(g["dev_" + key(n)]) <= 1e-5, (name, n)


def test_saturated_case_reaches_the_edge_of_the_focal_derivative():
    """`ties`: fp32 sigmoid of the saturated row's logits is exactly 1.0f for at least two columns."""
    z = golden("ties")["logits"][tc.SATURATED_ROW].astype(np.float32)
    assert int((torch.sigmoid(torch.from_numpy(z)).numpy() == np.float32(1.0)).sum()) >= 2


@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_eager_cpu_training_path_matches_the_goldens(name):
    c, g = tc.make_case(name), golden(name)
    m = S2DMatching(c["case"].C, thr=c["thr"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    m.train()
    d0 = torch.from_numpy(c["desc0"]).requires_grad_(True)
    d1 = torch.from_numpy(c["desc1"]).requires_grad_(True)
    data = m(d0, d1, {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"])})
    total = data["coarse_loss"] * c["g_loss"]
    if c["g_score"] is not None:
        total = total + (data["score_matrix"] * torch.from_numpy(c["g_score"])).sum()
    total.backward()
    assert abs(float(data["coarse_loss"].detach()) - float(g["loss"])) <= BAR * abs(float(g["loss"]))
    got = {"desc0": d0.grad, "desc1": d1.grad}
    got.update({n: p.grad for n, p in m.named_parameters()})
    for n in tc.GRAD_NAMES:
        assert rel(got[n].numpy(), g["grad_" + key(n)]) < max(BAR, 3 * float(g["dev_" + key(n)])), n


def test_hip_training_defaults_to_the_library_and_cpu_tensors_keep_the_eager_path():
    assert S2DMatching.hip_training is True
    m = S2DMatching(32).train()
    d0 = torch.randn(3, 32, requires_grad=True)
    data = m(d0, torch.randn(5, 32), {"conf_matrix_gt": torch.zeros(3, 5)})
    data["coarse_loss"].backward()
    assert d0.grad is not None and m.mlps[0].weight.grad is not None


def test_training_entry_points_validate_before_anything_is_dereferenced():
    """No GPU needed: the pointers below are host buffers that are never read."""
    lib = _lib.load()
    buf = (ct.c_char * 8192)()
    p = ct.cast(buf, ct.c_void_p)
    mis = ct.c_void_p(p.value + 4)
    F32, X3, BF, MX = (_lib.PRECISIONS[k] for k in ("fp32", "bf16x3", "bf16", "f16mx"))
    # size queries: 0 for an unsupported C or shape
    for C in (0, 16, 48, 288, -32):
        assert lib.nl_s2d_train_weights_bytes(C) == 0
        assert lib.nl_s2d_forward_train_workspace_bytes(8, 8, C) == 0
        assert lib.nl_s2d_backward_train_workspace_bytes(8, 8, C) == 0
    assert lib.nl_s2d_backward_train_workspace_bytes(0, 8, 64) == 0 and lib.nl_s2d_backward_train_workspace_bytes(1 << 20, 1 << 20, 64) == 0
    assert lib.nl_s2d_train_weights_bytes(192) > 0
    # the inference image is what it was
    assert lib.nl_s2d_packed_weights_bytes(192) == 2 * (2 * 192 * 128 * 2 + 2 * 32768) + 2048 + 192 * 128 * 4 + 128 * 128 * 4
    fneed = lib.nl_s2d_forward_train_workspace_bytes(4, 4, 64)
    bneed = lib.nl_s2d_backward_train_workspace_bytes(4, 4, 64)
    assert fneed > 0 and bneed > 0

    def fwd(packed=p, C=64, prec=X3, d0=p, N=4, d1=p, M=4, target=p, scores=p, logits=p, loss=p, mj=p, ms=p, ws=p, wsb=None):
        return lib.nl_s2d_forward_train(packed, C, prec, d0, N, d1, M, ct.c_float(0.2), target, scores, logits, loss, mj, ms, ws, fneed if wsb is None else wsb, None)
    for bad in (dict(packed=None), dict(d0=None), dict(d1=None), dict(scores=None), dict(logits=None), dict(mj=None), dict(ms=None), dict(N=-1), dict(M=0),
                dict(target=None), dict(loss=None), dict(d0=mis), dict(packed=mis), dict(prec=77), dict(C=0)):
        assert fwd(**bad) == _lib.NL_ERR_BAD_ARG, bad
    assert fwd(C=48) == _lib.NL_ERR_UNSUPPORTED and fwd(prec=MX) == _lib.NL_ERR_UNSUPPORTED
    assert fwd(wsb=fneed - 1) == _lib.NL_ERR_WORKSPACE and fwd(ws=None) == _lib.NL_ERR_WORKSPACE and fwd(ws=mis) == _lib.NL_ERR_WORKSPACE

    def bwd(packed=p, tp=p, C=64, prec=X3, d0=p, N=4, d1=p, M=4, logits=p, target=p, gl=p, gs=None, gd0=p, gd1=p, gp=(p,) * 6, ws=p, wsb=None):
        return lib.nl_s2d_backward_train(packed, tp, C, prec, d0, N, d1, M, logits, target, gl, gs, gd0, gd1, *gp, ws, bneed if wsb is None else wsb, None)
    for bad in (dict(packed=None), dict(tp=None), dict(d0=None), dict(d1=None), dict(logits=None), dict(gd0=None), dict(gd1=None), dict(N=0), dict(M=-3),
                dict(target=None), dict(gl=None), dict(tp=mis), dict(gd1=mis), dict(prec=-1), dict(C=-64)):
        assert bwd(**bad) == _lib.NL_ERR_BAD_ARG, bad
    assert bwd(C=80) == _lib.NL_ERR_UNSUPPORTED and bwd(prec=MX) == _lib.NL_ERR_UNSUPPORTED
    assert bwd(wsb=bneed - 1) == _lib.NL_ERR_WORKSPACE and bwd(ws=None) == _lib.NL_ERR_WORKSPACE and bwd(ws=mis) == _lib.NL_ERR_WORKSPACE
    for prec in (F32, BF):
        assert bwd(prec=prec, wsb=0) == _lib.NL_ERR_WORKSPACE   # a supported mode gets as far as the workspace check

    def pack(C=64, w1=p, w2=p, out=p, nbytes=None):
        return lib.nl_s2d_pack_train_weights(C, w1, w2, out, lib.nl_s2d_train_weights_bytes(64) if nbytes is None else nbytes, None)
    assert pack(w1=None) == _lib.NL_ERR_BAD_ARG and pack(w2=None) == _lib.NL_ERR_BAD_ARG and pack(out=None) == _lib.NL_ERR_BAD_ARG and pack(out=mis) == _lib.NL_ERR_BAD_ARG
    assert pack(C=0) == _lib.NL_ERR_BAD_ARG and pack(C=48) == _lib.NL_ERR_UNSUPPORTED and pack(nbytes=16) == _lib.NL_ERR_WORKSPACE
