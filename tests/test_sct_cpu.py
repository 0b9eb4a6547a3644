"""CPU-side tests of the SelfCrossTransformer drop-in (nerf_loc_amd/transformer.py): state-dict contract, the eager path and the restatement against the
reference's goldens, gradients, the no-CPU-fallback rule, and the argument checks of nl_sct_* that need no GPU."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import sct_cases as sc
from tests import sct_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bound(g):
    """How far an fp32 evaluation of the four layers may lie from the golden, as a share of the output's largest magnitude: 1e-6, or twice the reference's OWN fp32
    deviation from fp64 recorded in the golden where that is larger, never more than the 2e-6 tools/gen_sct_golden.py asserts for the restatement.  Both sides of
    the comparison are fp32 evaluations of the same formulas and each lies about that deviation from the fp64 result, so their distance reaches twice it: on
    `peaked` (recorded deviation 8.6e-7) the restatement measured 7.1e-7 against the golden on one host CPU and 1.04e-6 on another, deterministically on each.
    The other ten cases (deviations 1.3e-7 .. 3.8e-7) keep 1e-6.  DESIGN.md 5.31."""
    return min(2e-6, max(1e-6, 2.0 * float(g["ref_fp32_vs_fp64"].max())))


def _module(c, **kw):
    from nerf_loc_amd.transformer import SelfCrossTransformer
    case = c["case"]
    m = SelfCrossTransformer(d_model=case.C, nhead=sc.NHEAD, dim_feedforward=case.F, dropout=kw.pop("dropout", 0.1), activation="relu", **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=True)
    return m


def _inputs(c):
    return [torch.from_numpy(c[k]) for k in ("v0", "pos0", "v1", "pos1")]


def _rel(a, g):
    return float(np.abs(a.astype(np.float64) - g).max() / np.abs(g).max())


@pytest.mark.parametrize("name", sc.GOLDEN_CASES)
def test_state_dict_has_the_reference_names_and_shapes(name):
    g = sc.load_golden(GOLDEN, name)
    c = sc.make_case(name)
    sd = _module(c).state_dict()
    assert len(sd) == 52 and list(sd.keys()) == [str(n) for n in g["state_dict_names"]] == list(sc.STATE_NAMES)
    shapes = [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()]
    assert shapes == g["state_dict_shapes"].tolist()
    assert float(g["ref_fp32_vs_fp64"].max()) <= 1e-5


def test_matrices_are_xavier_initialised():
    from nerf_loc_amd.transformer import SelfCrossTransformer
    m = SelfCrossTransformer(d_model=64, nhead=8, dim_feedforward=128)
    w = m.self_attn_layer0.linear1.weight
    bound = float(np.sqrt(6.0 / (64 + 128)))
    amax = float(w.detach().abs().max())
    assert 0.9 * bound < amax <= bound


@pytest.mark.parametrize("name", sc.GOLDEN_CASES)
def test_eager_eval_and_restatement_equal_the_golden(name):
    c, g = sc.make_case(name), sc.load_golden(GOLDEN, name)
    m = _module(c).eval()
    with torch.no_grad():
        o0, o1 = m._eager(*_inputs(c))   # the eager formulation in eval mode (forward refuses CPU tensors there)
    assert o0.is_contiguous() and o1.is_contiguous()
    e = max(_rel(o0.numpy(), g["out0"]), _rel(o1.numpy(), g["out1"]))
    r = sr.forward(c, torch.float32)
    er = max(_rel(r[2], g["out0"]), _rel(r[3], g["out1"]))
    print(f"sct {name}: eager vs golden {e:.2e}, restatement fp32 vs golden {er:.2e} (bound {_bound(g):.2e})")
    assert e <= _bound(g) and er <= _bound(g)


def test_training_mode_without_dropout_equals_eval():
    c, g = sc.make_case("small"), sc.load_golden(GOLDEN, "small")
    m = _module(c, dropout=0.0).train()
    o0, o1 = m(*_inputs(c))
    assert o0.requires_grad
    assert max(_rel(o0.detach().numpy(), g["out0"]), _rel(o1.detach().numpy(), g["out1"])) <= _bound(g)


def test_every_applied_parameter_receives_a_gradient():
    c = sc.make_case("small")
    m = _module(c, dropout=0.0).eval()
    ins = _inputs(c)
    ins[0].requires_grad_(True)   # eval mode + an input under grad: the eager path
    o0, o1 = m(*ins)
    (o0.sum() + (o1 * o1).sum()).backward()
    unused = {f"cross_attn_layer{i}.norm1.{p}" for i in (0, 1) for p in ("weight", "bias")}
    for n, p in m.named_parameters():
        if n in unused:
            assert p.grad is None, n
        else:
            assert p.grad is not None and float(p.grad.abs().max()) > 0, n
    assert ins[0].grad is not None


def test_eval_on_cpu_tensors_raises():
    c = sc.make_case("one")
    m = _module(c).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(*_inputs(c))


def test_unsupported_configurations_have_no_packed_size():
    lib = _lib.load()
    assert lib.nl_sct_packed_bytes(192, 8, 512) > 0 and lib.nl_sct_packed_bytes(64, 8, 32) > 0
    assert lib.nl_sct_packed_bytes(192, 4, 512) == 0
    assert lib.nl_sct_packed_bytes(96, 8, 512) == 0
    assert lib.nl_sct_packed_bytes(192, 8, 520) == 0
    assert lib.nl_sct_packed_bytes(192, 8, 544) == 0
    assert lib.nl_sct_workspace_bytes(1, 1024, 4800, 192, 512) >= 4 * 4800 * 192 * 4
    assert lib.nl_sct_workspace_bytes(1, 0, 5, 192, 512) == 0


def test_arguments_are_validated_before_anything_is_dereferenced():
    """No GPU needed: the pointers are host buffers (or null) that a correct library never reads."""
    lib = _lib.load()
    buf = (ct.c_char * 8192)()
    p = ct.c_void_p((ct.addressof(buf) + 255) // 256 * 256)
    q = ct.c_void_p(p.value + 4)
    p2 = ct.c_void_p(p.value + 4096)
    need = lib.nl_sct_workspace_bytes(2, 5, 7, 64, 128)
    assert need > 0
    OK, BAD, UNS, WS = _lib.NL_OK, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE

    def fwd(packed=p, C=64, nhead=8, F=128, prec=1, v0=p, pos0=p, N0=5, v1=p, pos1=p, N1=7, B=2, out0=p, out1=p2, ws=p, ws_bytes=need):
        return lib.nl_sct_forward(packed, C, nhead, F, prec, v0, pos0, N0, v1, pos1, N1, B, out0, out1, ws, ws_bytes, None)

    def layer(packed=p, C=64, nhead=8, F=128, l=2, prec=1, x=p, xp=p, Nq=5, mem=p, mp=p, Nk=7, B=2, out=p, ws=p, ws_bytes=need):
        return lib.nl_sct_layer(packed, C, nhead, F, l, prec, x, xp, Nq, mem, mp, Nk, B, out, ws, ws_bytes, None)

    for call in (fwd, layer):
        assert call(ws=None) == WS and call(ws_bytes=need - 1) == WS and call(ws=q) == WS
        assert call(packed=None) == BAD and call(packed=q) == BAD
        assert call(B=-1) == BAD and call(prec=7) == BAD
        assert call(prec=_lib.PREC_F16MX) == UNS
        assert call(nhead=4) == UNS and call(C=96) == UNS and call(F=520) == UNS
        assert call(B=0, ws=None, packed=None) == OK   # nothing to do, nothing touched
    assert fwd(N0=0) == BAD and fwd(N1=-3) == BAD and fwd(v0=None) == BAD and fwd(pos1=None) == BAD and fwd(out1=None) == BAD and fwd(out0=q) == BAD
    assert fwd(B=1 << 20, N0=1 << 10) == UNS
    assert layer(l=4) == BAD and layer(l=-1) == BAD and layer(Nq=0) == BAD and layer(x=None) == BAD and layer(mem=None) == BAD and layer(out=None) == BAD
    assert layer(l=0, Nk=5, mem=q) == BAD and layer(l=1, Nk=7) == BAD   # self layers: the memory side is the target side
    assert lib.nl_sct_pack_weights(64, 8, 128, None, 52, p, 1 << 30, None) == BAD
    arr = (ct.c_void_p * 52)(*([p.value] * 52))
    assert lib.nl_sct_pack_weights(64, 8, 128, arr, 51, p, 1 << 30, None) == BAD
    assert lib.nl_sct_pack_weights(64, 8, 128, arr, 52, p, 16, None) == WS
    assert lib.nl_sct_pack_weights(64, 4, 128, arr, 52, p, 1 << 30, None) == UNS
