"""CPU-side tests of the SelfCrossTransformer training step: the gradient goldens against the fp64 restatement, the module's eager path against the goldens, the
argument checks and size queries of the ABI-13 entry points that need no GPU, the memory condition on the size queries, and the CPU fall-back of hip_training."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_train_cases as stc
from tests import sct_train_ref as str_

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4
KEYS = stc.INPUT_GRADS + stc.PARAM_NAMES
# softmax outputs (8 heads, fp32) that eager autograd keeps at (B 1, N0 1024, N1 4800): layers 0..3 = 1024^2, 4800^2, 1024 x 4800, 4800 x 1024 per head
EAGER_PROBABILITY_BYTES = 8 * 4 * (1024 * 1024 + 4800 * 4800 + 2 * 1024 * 4800)


@pytest.mark.parametrize("name", stc.GOLDEN_CASES)
def test_goldens_load_and_equal_the_restatement(name):
    """The files hold the fp32 rounding (2^-24 = 6e-8 of each element) of the reference's fp64 gradients, which the restatement meets to 1e-9 of a tensor's
    largest magnitude (tools/gen_sct_train_golden.py asserts that): so |golden - restatement| <= 1e-9 max |.| + 2^-24 |element|.  L is kept in fp64: 1e-9."""
    g = stc.load_grad_golden(GOLDEN, name)
    r = str_.grads(stc.make_case(name))
    assert abs(float(g["L"]) - r["L"]) <= 1e-9 * max(1.0, abs(r["L"]))
    assert all(r[n] is None for n in stc.UNUSED) and len(KEYS) == 52
    for k in KEYS:
        a, b = g[stc.key(k)], r[k]
        assert a.dtype == np.float32 and a.shape == b.shape, k
        assert (np.abs(a.astype(np.float64) - b) <= 1e-9 * np.abs(b).max() + 2.0 ** -24 * np.abs(b)).all(), k
        assert float(g["dev_" + stc.key(k)]) <= 3e-5, k
    if name == "one":   # a one-key softmax ignores q and k
        assert not g["g_pos0"].any() and not g["g_pos1"].any()


def _module(c, **kw):
    from nerf_loc_amd.transformer import SelfCrossTransformer
    case = c["case"]
    m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    return m


def _eager_grads(m, c):
    t = [torch.from_numpy(c[k]).requires_grad_(True) for k in ("v0", "pos0", "v1", "pos1")]
    o0, o1 = m._eager(*t)
    ((o0 * torch.from_numpy(c["g_out0"])).sum() + (o1 * torch.from_numpy(c["g_out1"])).sum()).backward()
    got = {k: x.grad.numpy() for k, x in zip(stc.INPUT_GRADS, t)}
    got.update({n: p.grad.numpy() for n, p in m.named_parameters() if p.grad is not None})
    return got


def test_eager_module_meets_the_goldens():
    c, g = stc.make_case("small"), stc.load_grad_golden(GOLDEN, "small")
    got = _eager_grads(_module(c).eval(), c)
    assert set(got) == set(KEYS)
    errs = {k: float(np.abs(got[k].astype(np.float64) - g[stc.key(k)]).max() / np.abs(g[stc.key(k)]).max()) for k in KEYS}
    k = max(errs, key=errs.get)
    print(f"sct eager gradients, small: worst max |error| / max |reference| {errs[k]:.2e} ({k})")
    assert errs[k] <= BAR


def test_hip_training_on_cpu_tensors_takes_the_eager_path():
    c = stc.make_case("small")
    m = _module(c, dropout=0.0).train()
    assert m.hip_training is False and m.dropout == 0.0
    m.hip_training = True
    o0, _ = m(*[torch.from_numpy(c[k]) for k in ("v0", "pos0", "v1", "pos1")])
    assert o0.requires_grad and m.pack_count == 0 and m._train_cache.pack_count == 0
    assert _module(c).dropout == 0.1   # the constructor's default, as the reference's


def test_size_queries_are_zero_for_what_the_calls_refuse():
    lib = _lib.load()
    assert lib.nl_abi_version() == 13
    assert lib.nl_sct_train_packed_bytes(192, 8, 512) > 0 and lib.nl_sct_train_packed_bytes(64, 8, 32) > 0
    for C, nhead, F in ((192, 4, 512), (96, 8, 512), (192, 8, 520), (192, 8, 544)):
        assert lib.nl_sct_train_packed_bytes(C, nhead, F) == 0
    for q in (lib.nl_sct_train_state_bytes, lib.nl_sct_backward_workspace_bytes, lib.nl_sct_layer_backward_workspace_bytes):
        assert q(1, 1024, 4800, 192, 512) > 0 and q(0, 5, 7, 64, 128) > 0
        assert q(1, 0, 5, 192, 512) == 0 and q(-1, 5, 5, 192, 512) == 0 and q(1, 5, 5, 96, 512) == 0 and q(1, 5, 5, 192, 520) == 0
        assert q(1 << 20, 1 << 10, 1, 192, 512) == 0   # beyond 2^24 rows


def test_memory_condition():
    """State + backward workspace stay below the softmax outputs eager keeps at the coarse shape, and doubling both sequences less than triples them: no
    heads x Nq x Nk term, which would give about four times."""
    lib = _lib.load()
    total = lambda n0, n1: lib.nl_sct_train_state_bytes(1, n0, n1, 192, 512) + lib.nl_sct_backward_workspace_bytes(1, n0, n1, 192, 512)
    a, b = total(1024, 4800), total(2048, 9600)
    print(f"sct training memory at (1, 1024, 4800, 192, 512): state + workspace {a / 1e6:.1f} MB against {EAGER_PROBABILITY_BYTES / 1e6:.1f} MB of eager softmax outputs; "
          f"at (2048, 9600): {b / 1e6:.1f} MB = {b / a:.2f} x")
    assert 1.08e9 <= EAGER_PROBABILITY_BYTES < 1.09e9
    assert a < 1.08e9
    assert b < 3 * a


def test_arguments_are_validated_before_anything_is_dereferenced():
    """No GPU needed: the pointers are host buffers (or null) that a correct library never reads."""
    lib = _lib.load()
    buf = (ct.c_char * 8192)()
    p = ct.c_void_p((ct.addressof(buf) + 255) // 256 * 256)
    q = ct.c_void_p(p.value + 4)
    p2 = ct.c_void_p(p.value + 4096)
    ws_f, sb, wb = lib.nl_sct_workspace_bytes(2, 5, 7, 64, 128), lib.nl_sct_train_state_bytes(2, 5, 7, 64, 128), lib.nl_sct_backward_workspace_bytes(2, 5, 7, 64, 128)
    lwb = lib.nl_sct_layer_backward_workspace_bytes(2, 5, 7, 64, 128)
    assert ws_f > 0 and sb > 0 and wb > 0 and lwb > wb
    OK, BAD, UNS, WS = _lib.NL_OK, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    grads = (ct.c_void_p * 52)(*([p.value] * 52))
    odd = (ct.c_void_p * 52)(*([p.value] * 51 + [q.value]))
    lgrads = (ct.c_void_p * 14)(*([p.value] * 14))

    def fwd(packed=p, C=64, nhead=8, F=128, prec=1, v0=p, pos0=p, N0=5, v1=p, pos1=p, N1=7, B=2, out0=p, out1=p2, state=p, state_bytes=sb, ws=p, ws_bytes=ws_f):
        return lib.nl_sct_forward_train(packed, C, nhead, F, prec, v0, pos0, N0, v1, pos1, N1, B, out0, out1, state, state_bytes, ws, ws_bytes, None)

    def bwd(packed=p, tp=p, C=64, nhead=8, F=128, prec=1, v0=p, pos0=p, N0=5, v1=p, pos1=p, N1=7, B=2, state=p, state_bytes=sb, g0=p, g1=p, gv0=p, gp0=p, gv1=p,
            gp1=p, grads=grads, n=52, ws=p, ws_bytes=wb):
        return lib.nl_sct_backward(packed, tp, C, nhead, F, prec, v0, pos0, N0, v1, pos1, N1, B, state, state_bytes, g0, g1, gv0, gp0, gv1, gp1, grads, n, ws, ws_bytes,
                                   None)

    def lay(packed=p, tp=p, C=64, nhead=8, F=128, l=2, prec=1, x=p, xp=p, Nq=5, mem=p, mp=p, Nk=7, B=2, g=p, gx=p, gxp=p, gm=p, gmp=p, grads=lgrads, n=14, ws=p,
            ws_bytes=lwb):
        return lib.nl_sct_layer_backward(packed, tp, C, nhead, F, l, prec, x, xp, Nq, mem, mp, Nk, B, g, gx, gxp, gm, gmp, grads, n, ws, ws_bytes, None)

    for call in (fwd, bwd, lay):
        assert call(ws=None) == WS and call(ws_bytes=16) == WS and call(ws=q) == WS
        assert call(packed=None) == BAD and call(packed=q) == BAD
        assert call(B=-1) == BAD and call(prec=7) == BAD
        assert call(prec=_lib.PREC_F16MX) == UNS
        assert call(nhead=4) == UNS and call(C=96) == UNS and call(F=520) == UNS
        assert call(B=0, ws=None, packed=None) == OK   # nothing to do, nothing touched
    assert fwd(N0=0) == BAD and fwd(v0=None) == BAD and fwd(out1=None) == BAD and fwd(out0=q) == BAD and fwd(B=1 << 20, N0=1 << 10) == UNS
    assert fwd(state=None) == WS and fwd(state_bytes=sb - 1) == WS and fwd(state=q) == WS
    assert bwd(tp=None) == BAD and bwd(tp=q) == BAD and bwd(N1=0) == BAD and bwd(pos0=None) == BAD and bwd(v1=q) == BAD and bwd(B=1 << 20, N0=1 << 10) == UNS
    assert bwd(gv0=q) == BAD and bwd(g1=q) == BAD and bwd(grads=odd) == BAD and bwd(n=48) == BAD
    assert bwd(state=None) == WS and bwd(state_bytes=sb - 1) == WS and bwd(ws_bytes=wb - 1) == WS
    assert lay(l=4) == BAD and lay(l=-1) == BAD and lay(Nq=0) == BAD and lay(x=None) == BAD and lay(mem=None) == BAD and lay(g=None) == BAD and lay(tp=None) == BAD
    assert lay(n=12) == BAD and lay(l=0, Nk=5, mem=None, mp=None, gm=None, gmp=None, n=14) == BAD   # a self layer has 12 tensors
    assert lay(l=0, Nk=5, mem=None, mp=None, n=12) == BAD                                            # ... and no memory-side gradient of its own
    assert lay(l=1, Nk=7, mem=None, mp=None, gm=None, gmp=None, n=12) == BAD                         # ... and Nk == Nq
    assert lay(ws_bytes=lwb - 1) == WS
    arr = (ct.c_void_p * 52)(*([p.value] * 52))
    assert lib.nl_sct_pack_weights_train(64, 8, 128, None, 52, p, 1 << 30, None) == BAD
    assert lib.nl_sct_pack_weights_train(64, 8, 128, arr, 51, p, 1 << 30, None) == BAD
    assert lib.nl_sct_pack_weights_train(64, 8, 128, arr, 52, q, 1 << 30, None) == BAD
    assert lib.nl_sct_pack_weights_train(64, 8, 128, arr, 52, p, 16, None) == WS
    assert lib.nl_sct_pack_weights_train(64, 4, 128, arr, 52, p, 1 << 30, None) == UNS
