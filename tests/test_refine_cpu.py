"""CPU-side tests of the pose refinement library's boundary (include/nerfloc_refine.h, nerf_loc_amd/_refine_lib.py) and of its two restatements — numpy
(tests/refine_ref.py) and differentiable torch (nerf_loc_amd/se3.py) — against tests/golden/refine_se3.npz, the outputs of the reference's se3_exp_map /
se3_log_map in fp64 (tools/gen_refine_golden.py).  Errors are max |a - b| / max |b| with b the reference's fp64 value: both sides evaluate the same formulas in
fp64, so values are held to 1e-12 and gradients to 1e-10."""
import ctypes as ct
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nerf_loc_amd import _cabi, _lib, _refine_lib, diff_render, se3
from tests import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerfloc_refine.h")
G = np.load(os.path.join(ROOT, "tests", "golden", "refine_se3.npz"))
NAMES = [str(n) for n in G["names"]]
VALUE_TOL, GRAD_TOL, ROUNDTRIP_TOL = 1e-12, 1e-10, 1e-10


def err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------------------------------ the seventh library's boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlr_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_refine_header_parses_through_the_binding_layer():
    P, I, L, Z, D, U = ct.c_void_p, ct.c_int, ct.c_int64, ct.c_size_t, ct.c_double, ct.c_uint
    protos = _cabi.prototypes("nerfloc_refine.h", "nlr_")
    assert protos == _refine_lib.SYMBOLS and len(protos) == 11
    assert sorted(n for n, _, _ in protos) == _declared()
    by_name = {n: (r, a) for n, r, a in protos}
    assert by_name["nlr_state_bytes"] == (Z, [I]) and by_name["nlr_init"] == (I, [P, U, I, P, P])   # typed out by hand
    assert by_name["nlr_se3_exp"] == (I, [P, L, P, P]) and by_name["nlr_se3_exp_backward"] == (I, [P, P, L, P, P])
    assert by_name["nlr_pose_rays"] == (I, [P, P, P, I, I, P, P, P, P, P])
    assert by_name["nlr_sample_target"] == (I, [P, I, I, I, I, I, I, P, I, P, P])
    assert by_name["nlr_loss"] == (I, [P, P, P, I, I, I, P, P, P])
    assert by_name["nlr_step"] == (I, [P, P, P, P, P, P, P, I, I, I, D, D, D, D, P])
    assert by_name["nlr_finish"] == (I, [P, I, P, P, P, P]) and not _cabi.struct_fields("nerfloc_refine.h")
    d = _cabi.defines("nerfloc_refine.h")
    assert d["NLR_MAX_POSES"] == 16 and d["NLR_STATE_DOUBLES"] == rr.STATE_DOUBLES == 44 and (d["NLR_POSE_F32"], d["NLR_POSE_F64"]) == (0, 1)


def test_refine_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_refine_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 11 and "nlr_step" in declared and "nlr_se3_log" in declared
    assert _exported(_refine_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no symbol of another library
    lib = _refine_lib.load()
    hdr = open(HEADER).read()
    assert lib.nlr_abi_version() == _refine_lib.ABI_VERSION == int(re.search(r"#define\s+NLR_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    assert not [n for n in _exported(_lib.LIB_PATH) if n.startswith("nlr_")]   # and the renderer's library holds none of it


def test_binding_describes_no_signature_by_hand():
    src = open(os.path.join(ROOT, "nerf_loc_amd", "_refine_lib.py")).read()
    assert "argtypes" not in src and "restype" not in src and "_cabi.bind(" in src


@pytest.fixture(scope="module")
def host():
    """(lib, p): p a 256-byte aligned HOST address that no call below may read — every call here is refused (or has nothing to do) before a launch."""
    buf = (ct.c_char * 8192)()
    return _refine_lib.load(), (ct.addressof(buf) + 255) // 256 * 256, buf


def test_state_bytes():
    lib = _refine_lib.load()
    assert lib.nlr_state_bytes(0) == 0 and lib.nlr_state_bytes(-1) == 0 and lib.nlr_state_bytes(17) == 0
    assert lib.nlr_state_bytes(1) == 44 * 8 and lib.nlr_state_bytes(16) == 16 * 44 * 8


def test_calls_refuse_bad_arguments_without_a_device(host):
    lib, p, _ = host
    BAD, UNS, OK = _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_UNSUPPORTED, _lib.NL_OK
    init = lambda poses=p, flags=0, B=2, state=p: lib.nlr_init(poses, flags, B, state, None)
    assert init(B=17) == UNS and init(B=-1) == BAD and init(flags=2) == BAD and init(poses=None) == BAD and init(state=None) == BAD
    assert init(poses=p + 4, flags=1) == BAD and init(state=p + 4) == BAD and init(B=0, poses=None, state=None) == OK
    rays = lambda state=p, K=p, uv=p, B=2, Rp=24, p32=p, o=p, d=p, c=p: lib.nlr_pose_rays(state, K, uv, B, Rp, p32, o, d, c, None)
    assert rays(B=17) == UNS and rays(Rp=-1) == BAD and rays(B=-1) == BAD and rays(Rp=(1 << 20) + 1) == UNS
    for null in ("state", "K", "uv", "o", "d", "c"):
        assert rays(**{null: None}) == BAD, null
    assert rays(o=p + 2) == BAD and rays(state=p + 4) == BAD
    assert rays(B=0, state=None) == OK and rays(Rp=0, uv=None) == OK   # nothing to do: nothing is dereferenced
    samp = lambda m=p, layout=0, C=3, h=5, w=7, H=32, W=48, uv=p, Rp=24, out=p: lib.nlr_sample_target(m, layout, C, h, w, H, W, uv, Rp, out, None)
    assert samp(C=0) == BAD and samp(C=1025) == UNS and samp(layout=2) == BAD and samp(h=0) == BAD and samp(W=0) == BAD and samp(Rp=-1) == BAD
    assert samp(m=None) == BAD and samp(uv=None) == BAD and samp(out=None) == BAD and samp(out=p + 1) == BAD and samp(Rp=0, m=None) == OK
    loss = lambda out=p, mask=p, tgt=p, B=2, Rp=24, C=5, g=p, rl=p: lib.nlr_loss(out, mask, tgt, B, Rp, C, g, rl, None)
    assert loss(B=17) == UNS and loss(Rp=-1) == BAD and loss(C=0) == BAD and loss(C=1025) == UNS and loss(C=0, B=0) == BAD
    for null in ("out", "mask", "tgt", "g", "rl"):
        assert loss(**{null: None}) == BAD, null
    assert loss(rl=p + 4) == BAD and loss(B=0, out=None) == OK and loss(Rp=0, out=None) == OK
    step = lambda state=p, rl=p, go=p, gd=p, gc=p, K=p, uv=p, B=2, Rp=24, C=5: lib.nlr_step(state, rl, go, gd, gc, K, uv, B, Rp, C, 1e-3, 0.9, 0.999, 1e-8, None)
    assert step(B=17) == UNS and step(Rp=-1) == BAD and step(C=0) == BAD
    for null in ("state", "rl", "go", "gd", "gc", "K", "uv"):
        assert step(**{null: None}) == BAD, null
    assert step(B=0, state=None) == OK and step(Rp=0, rl=None) == OK
    fin = lambda state=p, B=2, T64=p, T32=p, info=p: lib.nlr_finish(state, B, T64, T32, info, None)
    assert fin(B=17) == UNS and fin(B=-1) == BAD and fin(state=None) == BAD and fin(info=None) == BAD and fin(T64=p + 4) == BAD and fin(B=0, state=None) == OK
    for fn in (lib.nlr_se3_exp, lib.nlr_se3_log):
        assert fn(None, 3, p, None) == BAD and fn(p, 3, None, None) == BAD and fn(p, -1, p, None) == BAD and fn(p, (1 << 20) + 1, p, None) == UNS
        assert fn(None, 0, None, None) == OK
    assert lib.nlr_se3_exp_backward(p, None, 3, p, None) == BAD and lib.nlr_se3_exp_backward(None, None, 0, None, None) == OK


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(ValueError, match="HIP device"):
        _refine_lib.se3_exp(torch.zeros(2, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="1 <= B"):
        _refine_lib.new_state(17, "cpu")
    from nerf_loc_amd.pose_optimizer import PoseOptimizer
    with pytest.raises(NotImplementedError, match="SuperPoint"):
        PoseOptimizer(None, None, sampling='interest_region')
    with pytest.raises(RuntimeError, match="no CPU path"):
        PoseOptimizer(None, None).refine(torch.eye(4)[None], {})


# ------------------------------------------------------------------------------------------ the two restatements against the reference's fp64 values
@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_reproduces_the_reference(name):
    p, Gc, T, grad, lg, rt = [G[f"{name}.{k}"] for k in ("p", "G", "T", "grad", "log", "roundtrip")]
    assert err(rr.se3_exp(p), T) <= VALUE_TOL and err(rr.se3_log(T), lg) <= VALUE_TOL
    assert err(rr.se3_exp_backward(p, Gc), grad) <= GRAD_TOL
    back = rr.se3_exp(rr.se3_log(T))
    assert err(back, rt) <= ROUNDTRIP_TOL   # the reference's own round trip, everywhere
    assert sorted(G["roundtrip_exact"]) == ["angle_0p3", "angle_3p0", "far_translation", "zero_rotation"]   # pinned: the list in the file cannot switch the check off
    if name in G["roundtrip_exact"]:
        assert err(back, T) <= ROUNDTRIP_TOL
    else:   # at or below a clamp (squared angle 1e-4, cosine 1 - 1e-4) the round trip is NOT the matrix, for the reference either
        assert err(rt, T) > ROUNDTRIP_TOL
    assert float(G[f"{name}.dev_exp32"]) <= 1e-4 and float(G[f"{name}.dev_log32"]) <= 1e-4   # the generator's refusal bar


@pytest.mark.parametrize("name", NAMES)
def test_torch_se3_reproduces_the_reference(name):
    p, Gc, T, grad, lg, rt = [G[f"{name}.{k}"] for k in ("p", "G", "T", "grad", "log", "roundtrip")]
    pt = torch.tensor(p[None], requires_grad=True)
    Tt = se3.se3_exp_map(pt)
    (Tt * torch.from_numpy(Gc)).sum().backward()
    assert err(Tt.detach().numpy()[0], T) <= VALUE_TOL and err(pt.grad.numpy()[0], grad) <= GRAD_TOL
    lt = se3.se3_log_map(torch.from_numpy(T)[None])
    assert err(lt.numpy()[0], lg) <= VALUE_TOL and err(se3.se3_exp_map(lt).numpy()[0], rt) <= ROUNDTRIP_TOL
    assert Tt.dtype == torch.float64 and se3.se3_exp_map(pt.detach().float()).dtype == torch.float32


def test_cases_cover_both_sides_of_the_clamp_and_the_identity():
    assert set(NAMES) == {"zero_rotation", "below_clamp", "at_clamp", "angle_0p3", "angle_3p0", "far_translation"}
    ang = {n: float(np.linalg.norm(G[f"{n}.p"][3:])) for n in NAMES}
    assert ang["zero_rotation"] == 0 and abs(ang["below_clamp"] - 0.005) < 1e-15 and ang["at_clamp"] == 0.01 and abs(ang["angle_3p0"] - 3.0) < 1e-12
    assert np.abs(G["far_translation.p"][:3]).max() == 50.0 and sorted(G["below_clamp"]) == ["below_clamp", "zero_rotation"]
    for n in G["below_clamp"]:   # below the clamp no gradient flows through the angle: the rotation gradient is the matrices' share alone
        p, Gc = G[f"{n}.p"], G[f"{n}.G"]
        assert rr._coef(p[3:])["n"] < rr.EPS
    assert rr._coef(G["at_clamp.p"][3:])["n"] >= rr.EPS
    assert err(rr.se3_log(G["identity.T"]), G["identity.log"]) <= VALUE_TOL and np.abs(G["identity.log"]).max() == 0
    assert err(se3.se3_log_map(torch.from_numpy(G["identity.T"])[None]).numpy()[0] + 1.0, G["identity.log"] + 1.0) <= VALUE_TOL
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "refine_se3.npz")) < 32 * 1024


def test_adam_restatement_against_torch_optim():
    rng = np.random.default_rng(3)
    p0, grads = rng.standard_normal(6), rng.standard_normal((5, 6)) * np.array([1e-3, 1.0, 10.0, 1e-6, 0.1, 1.0])
    pt = torch.tensor(p0, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=2e-3, betas=(0.9, 0.999))
    s = rr.init_state(np.eye(4))
    s["params"] = p0.copy()
    for g in grads:
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        rr.adam(s, g, 2e-3, 0.9, 0.999, 1e-8)
        assert err(s["params"], pt.detach().numpy()) <= 1e-14
    st = opt.state[pt]
    assert s["t"] == 5 == int(st["step"]) and err(s["m"], st["exp_avg"].numpy()) <= 1e-14 and err(s["v"], st["exp_avg_sq"].numpy()) <= 1e-14


def test_ray_chain_and_its_backward_against_autograd_of_rays_from_pose():
    rng = np.random.default_rng(5)
    K = np.array([[40.0, 0, 23.5], [0, 42.0, 15.5], [0, 0, 1]], np.float32)
    uv = np.concatenate([rng.uniform(0, 47.9, (30, 1)), rng.uniform(0, 31.9, (30, 1))], 1).astype(np.float32)
    uv[:3] = [[0, 0], [47.99, 31.99], [12.5, 0.75]]
    T = G["angle_0p3.T"]
    o, d, c = rr.pose_rays(T, K, uv)
    pose = torch.tensor(T, requires_grad=True)
    ot, dt = diff_render.rays_from_pose(torch.from_numpy(uv), torch.from_numpy(K).double(), pose)
    assert err(o, ot.detach().numpy()) <= 1e-12 and err(d, dt.detach().numpy()) <= 1e-12 and np.array_equal(o, c)
    g_o, g_d, g_c = rng.standard_normal((3, 30, 3))
    (ot * torch.from_numpy(g_o + g_c)).sum().backward(retain_graph=True)
    (dt * torch.from_numpy(g_d)).sum().backward()
    Gm = rr.pose_rays_backward(T, K, uv, g_o, g_d, g_c)
    assert err(Gm[:3], pose.grad.numpy()[:3]) <= 1e-12 and not Gm[3].any()
    # and one whole step of the restatement against autograd through exp -> rays -> a linear functional, then torch.optim.Adam
    p0 = G["angle_0p3.p"]
    pt = torch.tensor(p0[None], requires_grad=True)
    opt = torch.optim.Adam([pt], lr=1e-3, betas=(0.9, 0.999))
    ot, dt = diff_render.rays_from_pose(torch.from_numpy(uv), torch.from_numpy(K).double(), se3.se3_exp_map(pt)[0])
    ((ot * torch.from_numpy(g_o + g_c)).sum() + (dt * torch.from_numpy(g_d)).sum()).backward()
    opt.step()
    s = rr.init_state(rr.se3_exp(p0))
    s["params"] = p0.copy()
    rr.step(s, np.full(30, 0.25), 5, g_o, g_d, g_c, K, uv, lr=1e-3)
    assert err(s["grad"], pt.grad.numpy()[0]) <= 1e-10 and err(s["params"], pt.detach().numpy()[0]) <= 1e-12
    assert s["loss_init"] == s["loss_last"] == 0.25 / 5 and s["t"] == 1 and not s["nan"]
    rr.step(s, np.array([0.5, np.nan]), 5, g_o[:2], g_d[:2], g_c[:2], K, uv[:2])
    before = s["params"].copy()
    rr.step(s, np.full(2, 0.1), 5, g_o[:2], g_d[:2], g_c[:2], K, uv[:2])   # latched: nothing moves any more
    assert s["nan"] == 1 and s["t"] == 1 and np.array_equal(before, s["params"]) and np.isnan(s["loss_last"]) and s["loss_init"] == 0.05
    assert np.array_equal(rr.finish(s)[0], s["pose0"]) and rr.finish(s)[1] == 0


def test_sample_target_restatement_against_interpolate():
    rng = np.random.default_rng(9)
    for (h, w), (H, W) in (((5, 7), (32, 48)), ((32, 48), (8, 12))):
        m = rng.standard_normal((3, h, w))
        full = torch.nn.functional.interpolate(torch.from_numpy(m)[None], size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
        uv = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2 + 0.7, H // 3 + 0.2]], np.float32)
        got = rr.sample_target(m, H, W, uv)
        want = full[:, uv[:, 1].astype(int), uv[:, 0].astype(int)].T
        assert err(got, want) <= 1e-12


def test_loss_restatement_against_torch_mean():
    rng = np.random.default_rng(11)
    out, tgt, mask = rng.standard_normal((7, 5)), rng.standard_normal((7, 5)), (rng.random(7) > 0.3)
    o = torch.tensor(out, requires_grad=True)
    loss = torch.mean(((o - torch.from_numpy(tgt)) * torch.from_numpy(mask).unsqueeze(1)) ** 2)
    loss.backward()
    rows, g = rr.loss_rows(out, mask, tgt)
    assert err(rows.sum() / 35, float(loss.detach())) <= 1e-14 and err(g, o.grad.numpy()) <= 1e-14
