"""CPU-side checks of the fine matcher (nerf_loc_amd/fine_matching.py, csrc/fine.hip): the test restatement tests/fine_ref.py reproduces the goldens the
reference itself produced, the drop-ins keep the reference's parameter names, the entry points refuse bad arguments before touching anything, the eval path
refuses CPU tensors, and the eager training path reproduces the reference's two losses."""
import ctypes as ct
import os
import warnings

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import fine_cases as fc
from tests import fine_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _modules(c, loss_type="l2_with_std", **kw):
    from nerf_loc_amd.fine_matching import FineMatching, FinePreprocess
    pre = FinePreprocess(fc.preprocess_config(c["case"]), **kw)
    pre.load_state_dict({k: torch.from_numpy(v) for k, v in c["proj"].items()}, strict=True)
    fm = FineMatching(fc.matching_config(c["case"], loss_type), **kw)
    fm.load_state_dict({k: torch.from_numpy(v) for k, v in c["mlp"].items()}, strict=True)
    return pre, fm


def _data(c):
    return {"stride_coarse": c["stride_coarse"], "stride_fine": c["stride_fine"], "b_ids": torch.from_numpy(c["b_ids"]), "j_ids": torch.from_numpy(c["j_ids"]),
            "mkps2d_c": torch.from_numpy(c["mkps2d_c"]), "expec_f_gt": torch.from_numpy(c["expec_f_gt"])}


@pytest.mark.parametrize("name", fc.GOLDEN_CASES)
def test_fine_ref_reproduces_the_reference_goldens(name):
    c, g = fc.make_case(name), fc.load_golden(GOLDEN, name)
    case = c["case"]
    assert g["feat_f1"].shape == (len(c["j_ids"]), 49, case.Cout)
    rows = fr.windows(c["feat_f"], c["b_ids"], c["j_ids"], case.s, c["proj"], torch.float32)
    err = np.abs(rows.astype(np.float64) - g["feat_f1"]).max() / np.abs(g["feat_f1"]).max()
    assert err <= 1e-6, err
    # the second stage on the reference's own rows, so that the ill-conditioned std of `peaked` sees the inputs the reference saw
    r = fr.match(c["feat_f0"], g["feat_f1"], c["mlp"], c["mkps2d_c"], torch.float32)
    assert np.abs(r["expec_f"].astype(np.float64) - g["expec_f"]).max() <= 1e-6
    assert np.abs(r["mkps2d_f"].astype(np.float64) - g["mkps2d_f"]).max() <= 1e-5   # key-points are tens of pixels: a few ulp
    assert np.abs(r["heatmap"].astype(np.float64) - g["heatmap"]).sum(axis=1).max() <= 1e-6
    assert str(g["kornia_source"]).startswith(("kornia", "stand-in"))
    # cells outside the map are the bias
    pad = fr.padded_cells(case.Hf, case.Wf, c["j_ids"], case.s)
    assert np.array_equal(g["feat_f1"][pad], np.broadcast_to(c["proj"]["proj.bias"], g["feat_f1"][pad].shape))
    if name == "borders":
        # a window with more padded than real cells; every cell but the centre is padded in some window (all four sides)
        assert pad.sum(axis=1).max() == 33 and np.array_equal(np.nonzero(~pad.any(axis=0))[0], [24])
    if name == "flat":   # uniform heat-map: coords 0, std = 2 sqrt(mean(g^2)) = 2 sqrt(4/9) = 4/3
        assert np.abs(g["expec_f"][:, :2]).max() <= 1e-6 and np.abs(g["expec_f"][:, 2] - 4.0 / 3.0).max() <= 1e-6


def test_std_sensitivity_stays_small_outside_the_peaked_case():
    """The generator's condition (tools/gen_fine_golden.py): except in `peaked`, at most 10 % of the matches have d_m > 1e-5, so the plain bar decides."""
    for name in fc.GOLDEN_CASES:
        c, g = fc.make_case(name), fc.load_golden(GOLDEN, name)
        d = fr.std_sensitivity(c["feat_f0"], g["feat_f1"], c["mlp"], c["mkps2d_c"])
        if name != "peaked":
            assert (d > 1e-5).mean() <= 0.10, name
        else:
            assert (g["heatmap"].max(axis=1) > 0.99).mean() > 0.5


def test_state_dicts_keep_the_reference_names_and_shapes():
    c, g = fc.make_case("c192"), fc.load_golden(GOLDEN, "c192")
    pre, fm = _modules(c)
    for m, key in ((pre, "pre"), (fm, "match")):
        sd = m.state_dict()
        assert list(sd.keys()) == [str(n) for n in g[key + "_state_dict_names"]]
        assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == g[key + "_state_dict_shapes"].tolist()
    from nerf_loc_amd.fine_matching import FinePreprocess
    cat = FinePreprocess({**fc.preprocess_config(c["case"]), "fine_concat_coarse_feat": True})
    assert sorted(cat.state_dict().keys()) == ["down_proj.bias", "down_proj.weight", "merge_feat.bias", "merge_feat.weight"]
    assert tuple(cat.merge_feat.weight.shape) == (192, 384) and tuple(cat.down_proj.weight.shape) == (192, 384)
    with pytest.raises(ValueError):
        FinePreprocess(fc.preprocess_config(c["case"]), precision="fp8")


def test_packed_bytes_and_argument_checks_need_no_gpu():
    lib = _lib.load()
    for Cw in (16, 48, 288):
        assert lib.nl_fine_proj_packed_bytes(Cw, 64) == 0 and lib.nl_fine_proj_packed_bytes(64, Cw) == 0
    for Cw in (32, 192, 256):
        assert lib.nl_fine_proj_packed_bytes(Cw, Cw) >= Cw * Cw * 8 + Cw * 4
    buf = (ct.c_char * 4096)()
    p = ct.cast(buf, ct.c_void_p).value
    p = (p + 15) // 16 * 16
    OK, BAD, UNS, WSP = _lib.NL_OK, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_WORKSPACE
    X3 = _lib.PREC_BF16X3

    def pk(Cf=64, Cout=64, w=p, b=p, out=p, n=None):
        return lib.nl_fine_pack_proj(Cf, Cout, w, b, out, lib.nl_fine_proj_packed_bytes(64, 64) if n is None else n, None)
    assert pk(Cf=48) == BAD and pk(Cout=288) == BAD and pk(w=None) == BAD and pk(b=None) == BAD and pk(out=None) == BAD and pk(out=p + 4) == BAD
    assert pk(n=lib.nl_fine_proj_packed_bytes(64, 64) - 1) == WSP

    def win(packed=p, Cf=64, Cout=64, prec=X3, feat=p, B=1, Hf=8, Wf=8, b=p, j=p, M=4, stride=2, out=p):
        return lib.nl_fine_windows(packed, Cf, Cout, prec, feat, B, Hf, Wf, b, j, M, stride, out, None)
    for bad in (dict(packed=None), dict(feat=None), dict(b=None), dict(j=None), dict(out=None), dict(M=-1), dict(Cf=16), dict(Cout=48), dict(Cf=288),
                dict(stride=0), dict(stride=-2), dict(B=0), dict(Hf=0), dict(prec=7), dict(feat=p + 4), dict(j=p + 4)):
        assert win(**bad) == BAD, bad
    assert win(prec=_lib.PREC_F16MX) == UNS
    assert win(M=0) == OK and win(M=0, packed=None, feat=None, b=None, j=None, out=None) == OK       # nothing launched, nothing dereferenced
    assert win(M=0, stride=0) == BAD and win(M=0, Cf=48) == BAD

    def mt(packed=p, C=64, prec=X3, f0=p, f1=p, M=4, kc=p, ex=p, kf=p, heat=None):
        return lib.nl_fine_match(packed, C, prec, f0, f1, M, kc, ex, kf, heat, None)
    for bad in (dict(packed=None), dict(f0=None), dict(f1=None), dict(kc=None), dict(ex=None), dict(kf=None), dict(M=-1), dict(C=16), dict(C=48), dict(C=288),
                dict(prec=-1), dict(f1=p + 8), dict(heat=p + 2)):
        assert mt(**bad) == BAD, bad
    assert mt(prec=_lib.PREC_F16MX) == UNS
    assert mt(M=0) == OK and mt(M=0, packed=None, f0=None, f1=None, kc=None, ex=None, kf=None) == OK
    assert mt(M=0, C=48) == BAD


def test_eval_mode_refuses_cpu_tensors_and_handles_no_matches():
    c = fc.make_case("small")
    pre, fm = _modules(c)
    pre.eval(), fm.eval()
    data = _data(c)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pre(torch.from_numpy(c["feat_f"]), None, data)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fm(torch.from_numpy(c["feat_f0"]), torch.zeros(len(c["j_ids"]), 49, 64), data)
        # no coarse matches: the shapes and keys of the reference, on any device
        empty = {**data, "j_ids": torch.zeros(0, dtype=torch.int64), "b_ids": torch.zeros(0, dtype=torch.int64), "mkps2d_c": torch.zeros(0, 2)}
        f1 = pre(torch.from_numpy(c["feat_f"]), None, empty)
        assert tuple(f1.shape) == (0, 49, 64)
        assert fm(torch.zeros(0, 64), f1, empty) is None
        assert tuple(empty["expec_f"].shape) == (0, 3) and empty["mkps2d_f"] is empty["mkps2d_c"]


def test_eager_training_path_reproduces_the_reference_losses():
    c = fc.make_case(fc.TRAIN_CASE)
    want = np.load(os.path.join(GOLDEN, "fine_train.npz"))
    g = fc.load_golden(GOLDEN, fc.TRAIN_CASE)
    for lt in fc.LOSS_TYPES:
        pre, fm = _modules(c, lt)
        pre.train(), fm.train()
        data = _data(c)
        f1 = pre(torch.from_numpy(c["feat_f"]), None, data)
        assert f1.requires_grad and np.abs(f1.detach().numpy() - g["feat_f1"]).max() <= 1e-6 * np.abs(g["feat_f1"]).max()
        out = fm(torch.from_numpy(c["feat_f0"]), f1, data)
        assert out is data and data["fine_loss"].requires_grad and not data["mkps2d_f"].requires_grad
        ref = float(want["fine_loss_" + lt])
        assert abs(data["fine_loss"].item() - ref) <= 1e-5 * abs(ref), (lt, data["fine_loss"].item(), ref)
        assert np.abs(data["expec_f"].detach().numpy() - g["expec_f"]).max() <= 1e-6
        assert abs(fr.losses(g["expec_f"], c["expec_f_gt"], fc.TRAIN_CORRECT_THR)[lt] - ref) <= 1e-5 * abs(ref)
        data["fine_loss"].backward()
        assert pre.proj.weight.grad is not None and fm.mlps[0].weight.grad is not None


def test_no_correct_match_branch_warns_and_stays_finite():
    c = fc.make_case(fc.TRAIN_CASE)
    for lt in fc.LOSS_TYPES:
        pre, fm = _modules(c, lt)
        pre.train(), fm.train()
        data = _data(c)
        data["expec_f_gt"] = torch.full_like(data["expec_f_gt"], 5.0)     # nothing within correct_thr
        f1 = pre(torch.from_numpy(c["feat_f"]), None, data)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fm(torch.from_numpy(c["feat_f0"]), f1, data)
        assert any("no correct coarse match" in str(x.message) for x in w)
        assert torch.isfinite(data["fine_loss"])
        if lt == "l2_with_std":
            assert data["fine_loss"].item() == 0.0                         # the one false supervision carries weight 0
        fm.eval()
        assert fm.get_loss(data["expec_f"].detach(), data["expec_f_gt"]) is None


def test_concatenated_coarse_features_take_the_eager_formulation():
    """fine_concat_coarse_feat=True (fine_matching.py:59-65) has no kernel: eager PyTorch on any device, eval mode included, equal to the formulation written out."""
    from nerf_loc_amd.fine_matching import FinePreprocess, gather_windows
    c = fc.make_case("small")
    case = c["case"]
    torch.manual_seed(0)
    m = FinePreprocess({**fc.preprocess_config(case), "fine_concat_coarse_feat": True}).eval()
    Ly, Lx = fc.grid_shape(case.Hf, case.Wf, case.s)
    feat_c1 = torch.randn(case.B, 2 * case.Cf, Ly, Lx)
    data = _data(c)
    with torch.no_grad():
        out = m(torch.from_numpy(c["feat_f"]), feat_c1, data)
        win = gather_windows(torch.from_numpy(c["feat_f"]), data["b_ids"], data["j_ids"], case.s)
        assert np.array_equal(win.numpy(), fr.windows(c["feat_f"], c["b_ids"], c["j_ids"], case.s))
        pick = feat_c1.flatten(2)[data["b_ids"], :, data["j_ids"]]
        want = m.merge_feat(torch.cat([m.down_proj(pick)[:, None].repeat(1, 49, 1), win], dim=2))
    assert tuple(out.shape) == (len(c["j_ids"]), 49, case.Cout) and torch.equal(out, want)
