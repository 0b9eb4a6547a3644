"""CPU-side checks of the fine matcher's training step (nerf_loc_amd/fine_matching.py, csrc/fine_bwd.hip): the fp64 restatement tests/fine_train_ref.py reproduces
the gradients the reference itself produced, the recipes keep clear of the std clamp wherever a std cotangent flows, the new entry points refuse bad arguments
before anything is dereferenced, and CPU tensors in training mode keep the eager path and match the reference's loss gradients."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import fine_train_cases as tc
from tests import fine_train_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("name", tc.GOLDEN_CASES)
def test_restatement_reproduces_the_reference_goldens(name):
    c, g = tc.make_case(name), tc.load_grad_golden(GOLDEN, name)
    r = ref.train_step(c)
    assert rel(r["expec_f"], g["expec_f"]) <= 1e-9
    for n in tc.GRAD_NAMES:
        want = g["grad_" + tc.key(n)]
        assert r["grads"][n].shape == want.shape, n
        if n == "mlps.4.bias":
            # softmax ignores a common shift of the logits: this gradient is zero up to rounding in the reference (1e-17) and in the restatement alike
            scale = float(np.abs(ref.match_backward(c["feat_f0"], r["feat_f1"], c["mlp"], c["g_expec"])["g_logit"]).sum())
            assert abs(float(r["grads"][n][0])) <= 1e-12 * max(scale, 1e-300) and abs(float(want[0])) <= 1e-12 * max(scale, 1e-300)
        elif name == "flat" and n in tc.FLAT_ZERO:
            assert not want.any() and not r["grads"][n].any(), n
        else:
            assert rel(r["grads"][n], want) <= 1e-9, n


def test_std_cotangent_flows_only_where_the_variance_stays_clear_of_the_clamp():
    """The generator's condition: a non-zero std cotangent needs every per-axis variance above MIN_VARIANCE; `peaked` (down to 3e-16) has a zero std cotangent."""
    for name in tc.GOLDEN_CASES:
        c, g = tc.make_case(name), tc.load_grad_golden(GOLDEN, name)
        vmin = ref.min_variance(c["feat_f0"], ref.train_step(c)["feat_f1"], c["mlp"])
        assert abs(vmin - float(g["min_variance"])) <= 1e-9 * max(abs(vmin), 1e-12)
        if name in tc.ZERO_STD_COTANGENT:
            assert not c["g_expec"][:, 2].any() and vmin < 1e-10
        else:
            assert c["g_expec"][:, 2].any() and vmin > tc.MIN_VARIANCE, (name, vmin)
            assert vmin >= (3.1e-3 if name == "s1" else 1.3e-2), (name, vmin)   # thirty times the condition and more: s1 is the lowest (3.2e-3)


def test_backward_entry_points_validate_before_anything_is_dereferenced():
    """No GPU needed: the pointers below are host buffers that are never read."""
    lib = _lib.load()
    buf = (ct.c_char * 8192)()
    p = ct.c_void_p((ct.cast(buf, ct.c_void_p).value + 15) // 16 * 16)
    mis = ct.c_void_p(p.value + 4)
    BAD, UNS, WSP, OK = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE, _lib.NL_OK
    F32, X3, BF, MX = (_lib.PRECISIONS[k] for k in ("fp32", "bf16x3", "bf16", "f16mx"))
    # size queries: 0 for unsupported widths or shapes, and what the header documents otherwise
    for C in (0, 16, 48, 288, -32):
        assert lib.nl_fine_match_backward_workspace_bytes(8, C) == 0
        assert lib.nl_fine_windows_backward_workspace_bytes(C, 64, 1, 8, 8, 2, 8) == 0 and lib.nl_fine_windows_backward_workspace_bytes(64, C, 1, 8, 8, 2, 8) == 0
        assert lib.nl_fine_proj_train_bytes(C, 64) == 0 and lib.nl_fine_proj_train_bytes(64, C) == 0
    assert lib.nl_fine_match_backward_workspace_bytes(-1, 64) == 0 and lib.nl_fine_match_backward_workspace_bytes(1 << 20, 64) == 0
    top = _lib.FINE_BACKWARD_MAX_M   # the modules take the eager path above it: the two must agree
    assert f"#define NL_FINE_BACKWARD_MAX_M {top}" in open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "nerfloc_render.h")).read()
    assert lib.nl_fine_match_backward_workspace_bytes(top, 64) > 0 and lib.nl_fine_match_backward_workspace_bytes(top + 1, 64) == 0
    assert lib.nl_fine_windows_backward_workspace_bytes(64, 64, 1, 8, 8, 2, top) > 0 and lib.nl_fine_windows_backward_workspace_bytes(64, 64, 1, 8, 8, 2, top + 1) == 0
    assert lib.nl_fine_windows_backward_workspace_bytes(64, 64, 1, 8, 8, 0, 8) == 0 and lib.nl_fine_windows_backward_workspace_bytes(64, 64, 0, 8, 8, 2, 8) == 0
    assert lib.nl_fine_proj_train_bytes(64, 96) == 64 * 96 * 8 + 64 * 4
    assert lib.nl_fine_proj_packed_bytes(64, 96) == 64 * 96 * 8 + 96 * 4      # the inference image is what it was
    mneed = lib.nl_fine_match_backward_workspace_bytes(100, 192)
    assert 100 * 49 * (192 + 384) * 4 <= mneed <= 100 * 49 * (192 + 384) * 4 + 256 * 128 * 193 * 4 + 128 * 256 * 4 + 100 * 132 * 4 + 8 * 256
    wneed = lib.nl_fine_windows_backward_workspace_bytes(64, 96, 2, 12, 16, 2, 100)
    assert 100 * 49 * 64 * 8 <= wneed <= 100 * 49 * 64 * 8 + 256 * (96 * 64 + 96) * 4 + 96 * 64 * 4 + (200 + 2 * 6 * 8 + 1) * 4 + 8 * 256

    mn = lib.nl_fine_match_backward_workspace_bytes(4, 64)

    def mb(packed=p, tp=p, C=64, prec=X3, f0=p, f1=p, M=4, heat=p, ge=p, gf0=p, gf1=p, gp=(p,) * 6, ws=p, wsb=None):
        return lib.nl_fine_match_backward(packed, tp, C, prec, f0, f1, M, heat, ge, gf0, gf1, *gp, ws, mn if wsb is None else wsb, None)
    for bad in (dict(packed=None), dict(tp=None), dict(f0=None), dict(f1=None), dict(heat=None), dict(ge=None), dict(M=-1), dict(C=16), dict(C=48), dict(C=288),
                dict(prec=9), dict(tp=mis), dict(f1=mis), dict(gf0=mis), dict(heat=ct.c_void_p(p.value + 2))):
        assert mb(**bad) == BAD, bad
    assert mb(prec=MX) == UNS and mb(M=1 << 20) == UNS
    assert mb(wsb=mn - 1) == WSP and mb(ws=None) == WSP and mb(ws=mis) == WSP
    for prec in (F32, BF):
        assert mb(prec=prec, wsb=0) == WSP   # a supported mode gets as far as the workspace check
    assert mb(gf0=None, gf1=None, gp=(None,) * 6, wsb=0) == WSP   # every output may be NULL
    assert mb(M=0) == OK and mb(M=0, packed=None, tp=None, f0=None, f1=None, heat=None, ge=None, ws=None, wsb=0) == OK   # nothing launched
    assert mb(M=0, C=48) == BAD

    wn = lib.nl_fine_windows_backward_workspace_bytes(64, 64, 1, 8, 8, 2, 4)

    def wb(packed=p, tp=p, Cf=64, Cout=64, prec=X3, feat=p, B=1, Hf=8, Wf=8, b=p, j=p, M=4, stride=2, go=p, gw=p, gb=p, gm=p, ws=p, wsb=None):
        return lib.nl_fine_windows_backward(packed, tp, Cf, Cout, prec, feat, B, Hf, Wf, b, j, M, stride, go, gw, gb, gm, ws, wn if wsb is None else wsb, None)
    for bad in (dict(packed=None), dict(tp=None), dict(feat=None), dict(b=None), dict(j=None), dict(go=None), dict(M=-1), dict(Cf=16), dict(Cout=48), dict(Cf=288),
                dict(stride=0), dict(stride=-2), dict(B=0), dict(Hf=0), dict(prec=7), dict(feat=mis), dict(j=mis), dict(go=mis), dict(gm=mis), dict(tp=mis)):
        assert wb(**bad) == BAD, bad
    assert wb(prec=MX) == UNS and wb(M=1 << 20) == UNS
    assert wb(wsb=wn - 1) == WSP and wb(ws=None) == WSP and wb(ws=mis) == WSP
    assert wb(gw=None, gb=None, gm=None, wsb=0) == WSP
    assert wb(M=0, stride=0) == BAD and wb(M=0, Cf=48) == BAD
    assert wb(M=0, gw=None, gb=None, gm=None, packed=None, tp=None, feat=None, b=None, j=None, go=None, ws=None, wsb=0) == OK   # no pointer given: nothing written

    def pk(Cf=64, Cout=64, w=p, out=p, n=None):
        return lib.nl_fine_pack_proj_train(Cf, Cout, w, out, lib.nl_fine_proj_train_bytes(64, 64) if n is None else n, None)
    assert pk(Cf=48) == BAD and pk(Cout=288) == BAD and pk(w=None) == BAD and pk(out=None) == BAD and pk(out=mis) == BAD
    assert pk(n=lib.nl_fine_proj_train_bytes(64, 64) - 1) == WSP


def _modules(c, loss_type):
    from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess
    pre = FinePreprocess(tc.fc.preprocess_config(c["case"]))
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    fm = FineMatching(tc.fc.matching_config(c["case"], loss_type))
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
    return pre.train(), fm.train()


@pytest.mark.parametrize("loss_type", tc.LOSS_TYPES)
def test_cpu_tensors_in_training_mode_keep_the_eager_path_and_match_the_loss_goldens(loss_type):
    from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess
    assert FinePreprocess.hip_training is True and FineMatching.hip_training is True   # the measured default (profiles/fine_train_bench.jsonl)
    c, g = tc.make_case(tc.TRAIN_CASE), tc.load_grad_golden(GOLDEN, tc.TRAIN_CASE)
    pre, fm = _modules(c, loss_type)
    pre.hip_training = fm.hip_training = True   # CPU tensors take the eager path whatever the switch says
    feat_f = torch.from_numpy(c["feat_f"]).requires_grad_(True)
    feat_f0 = torch.from_numpy(c["feat_f0"]).requires_grad_(True)
    data = {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": torch.from_numpy(c["b_ids"]), "j_ids": torch.from_numpy(c["j_ids"]),
            "mkps2d_c": torch.from_numpy(c["mkps2d_c"]), "expec_f_gt": torch.from_numpy(c["expec_f_gt"])}
    fm(feat_f0, pre(feat_f, None, data), data)
    want_loss = float(g["loss_" + loss_type])
    assert abs(float(data["fine_loss"].detach()) - want_loss) <= 1e-5 * abs(want_loss)
    data["fine_loss"].backward()
    got = {"feat_f": feat_f.grad, "feat_f0": feat_f0.grad}
    got.update({n: q.grad for n, q in list(pre.named_parameters()) + list(fm.named_parameters())})
    for n in tc.GRAD_NAMES:
        if n == "mlps.4.bias":   # zero up to rounding (see above): autograd's noise there is held to the scale of its neighbour mlps.4.weight; the library writes 0
            assert abs(float(got[n][0])) <= 1e-4 * float(got["mlps.4.weight"].abs().max())
            continue
        e, bound = rel(got[n].numpy(), g[f"lossgrad_{loss_type}_{tc.key(n)}"]), max(BAR, 3 * float(g[f"lossdev_{loss_type}_{tc.key(n)}"]))
        assert e < bound, (n, e, bound)
