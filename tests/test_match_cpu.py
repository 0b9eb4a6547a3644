"""CPU-side checks of the coarse matcher (nerf_loc_amd/matching.py, csrc/s2d.hip): the test restatement tests/match_ref.py reproduces the goldens the
reference produced, the module keeps the reference's state_dict contract and its training-mode loss, and the C-ABI refuses bad arguments before any launch."""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from nerf_loc_amd import _lib
from tests import match_cases as mc
from tests import match_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"s2d_{name}.npz"))


@pytest.mark.parametrize("name", mc.GOLDEN_CASES)
def test_match_ref_reproduces_the_reference_goldens(name):
    """score_matrix to 1e-5 absolute (both sides fp32 torch on the CPU; the allowance covers a different GEMM blocking under row chunking), i_ids / j_ids equal
    on decided rows (eps = 2e-4, the GPU test's definition)."""
    c, g = mc.make_case(name), _golden(name)
    s = mr.scores(c["desc0"], c["desc1"], c["weights"], torch.float32)
    err = np.abs(s.astype(np.float64) - g["score_matrix"].astype(np.float64)).max()
    print(f"{name}: max |s - s_golden| = {err:.3e}")
    assert err <= 1e-5
    mj = mr.select(s, c["thr"])
    ref_j = np.full(c["case"].N, -1, dtype=np.int64)
    ref_j[g["i_ids"]] = g["j_ids"]
    decided = ~mr.undecided_rows(g["score_matrix"], c["thr"], 2e-4)
    assert np.array_equal(mj[decided], ref_j[decided])
    # the selection rule itself, on the golden's own scores: exact for every row, the ties included
    assert np.array_equal(mr.select(g["score_matrix"], c["thr"]), ref_j)


def test_ties_case_holds_the_ties_it_was_built_for():
    g = _golden("ties")
    s = g["score_matrix"]
    assert int((s[7] == np.float32(1.0)).sum()) >= 2                       # sigmoid saturation: tied at 1.0f
    assert np.array_equal(s[:, 10], s[:, 11]) and np.array_equal(s[:, 10], s[:, 300])   # three byte-identical columns
    assert np.array_equal(s[20], s[21])                                    # two byte-identical rows
    ref_j = np.full(s.shape[0], -1, dtype=np.int64)
    ref_j[g["i_ids"]] = g["j_ids"]
    assert ref_j[5] == 10 and ref_j[20] == ref_j[21] >= 0                  # first of the tied columns; both tied rows keep the column


def test_module_state_dict_contract_and_training_loss():
    from nerf_loc_amd.matching import S2DMatching
    g = _golden("small")
    m = S2DMatching(192, thr=0.2)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in g["state_dict_names"]] == list(mc.PARAM_NAMES)
    for v, shp in zip(sd.values(), g["state_dict_shapes"]):
        assert list(v.shape) == [int(x) for x in shp[:v.dim()]]
    c = mc.make_case("small")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["weights"].items()}, strict=True)
    m.train()
    data = {"conf_matrix_gt": torch.from_numpy(c["conf_matrix_gt"])}
    m(torch.from_numpy(c["desc0"]), torch.from_numpy(c["desc1"]), data)
    want = float(np.load(os.path.join(GOLDEN, "s2d_train.npz"))["coarse_loss"])
    got = float(data["coarse_loss"].detach())
    print(f"coarse_loss {got:.9e} vs golden {want:.9e}")
    assert abs(got - want) <= 1e-5 * abs(want)
    assert data["coarse_loss"].requires_grad
    assert data["score_matrix"].shape == (96, 600) and data["i_ids"].dtype == torch.int64 and data["j_ids"].dtype == torch.int64
    assert np.array_equal(data["i_ids"].numpy(), g["i_ids"]) and np.array_equal(data["j_ids"].numpy(), g["j_ids"])


def test_eval_on_cpu_tensors_is_refused():
    from nerf_loc_amd.matching import S2DMatching
    m = S2DMatching(192).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 192), torch.zeros(8, 192), {})


def test_abi_binds_the_matcher_and_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 8 and lib.nl_abi_version() == _lib.ABI_VERSION
    for C in (0, 16, 100, 288, -32):
        assert lib.nl_s2d_packed_weights_bytes(C) == 0
    b192, b256 = lib.nl_s2d_packed_weights_bytes(192), lib.nl_s2d_packed_weights_bytes(256)
    assert 0 < b192 < b256 < (1 << 20)
    assert lib.nl_s2d_min_workspace_bytes(0, 10, 192, 1) == 0 and lib.nl_s2d_min_workspace_bytes(10, 0, 192, 1) == 0
    assert lib.nl_s2d_min_workspace_bytes(10, 10, 100, 1) == 0
    w1 = lib.nl_s2d_min_workspace_bytes(1024, 4800, 192, 1)
    w0 = lib.nl_s2d_min_workspace_bytes(1024, 4800, 192, 0)
    assert 0 < w1 < 64 * 1024 and w0 >= w1 + 1024 * 4800 * 4
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 15) & ~15   # host memory, 16-byte aligned, never dereferenced: every call below is refused before a launch

    def match(packed=p, C=192, prec=_lib.PREC_BF16X3, d0=p, N=4, d1=p, M=4, scores=p, mj=p, ms=p, ws=p, ws_bytes=8192):
        return lib.nl_s2d_match(packed, C, prec, d0, N, d1, M, ct.c_float(0.2), scores, mj, ms, ws, ws_bytes, None)
    assert match(N=0) == _lib.NL_ERR_BAD_ARG and match(M=0) == _lib.NL_ERR_BAD_ARG and match(N=-3) == _lib.NL_ERR_BAD_ARG
    assert match(C=100) == _lib.NL_ERR_UNSUPPORTED and match(C=288) == _lib.NL_ERR_UNSUPPORTED
    assert match(prec=_lib.PREC_F16MX) == _lib.NL_ERR_UNSUPPORTED
    assert match(prec=17) == _lib.NL_ERR_BAD_ARG
    for k in ("packed", "d0", "d1", "mj", "ms"):
        assert match(**{k: None}) == _lib.NL_ERR_BAD_ARG, k
    assert match(d0=p + 4) == _lib.NL_ERR_BAD_ARG            # descriptors are read as 16-byte pieces
    need = lib.nl_s2d_min_workspace_bytes(4, 4, 192, 1)
    assert match(ws_bytes=need - 1) == _lib.NL_ERR_WORKSPACE and match(ws=None) == _lib.NL_ERR_WORKSPACE
    need0 = lib.nl_s2d_min_workspace_bytes(4, 4, 192, 0)
    assert need0 > need and match(scores=None, ws_bytes=need0 - 1) == _lib.NL_ERR_WORKSPACE
    # packing
    pk = lambda **kw: lib.nl_s2d_pack_weights(kw.get("C", 192), kw.get("w1", p), p, p, p, p, p, kw.get("out", p), kw.get("n", b192), None)
    assert pk(C=100) == _lib.NL_ERR_UNSUPPORTED and pk(w1=None) == _lib.NL_ERR_BAD_ARG and pk(out=None) == _lib.NL_ERR_BAD_ARG
    assert pk(n=b192 - 1) == _lib.NL_ERR_WORKSPACE
