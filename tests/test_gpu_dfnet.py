"""The per-frame encoder of libnerfloc_cnn.so on the GPU: nlc_dfnet_forward against the reference's fp64 fixtures (tests/golden/dfnet_*.npz) and against the fp64
restatement of its header, its determinism and view independence, its refusals, and the opt-in path of DepthFusionNet / ConditionalNeRF.

The bar per tensor is the project's: max |err| / max |ref| <= 1e-4.  Where the fixture records that the reference's OWN fp32 run misses its fp64 run by more than
1.25e-5 on a tensor (`fp32_dev_<tensor>`), the bar is 8 x that recorded value, the guard factor of the geometry fixtures: such a tensor is ill-conditioned on that
recipe (min32's 2 x 2 planes under InstanceNorm).  The bar is read from the file, never from the code under test."""
import ctypes as ct
import functools
import os

import numpy as np
import pytest
import torch

from tests import dfnet_cases as dc
from tests import dfnet_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR, GUARD, FACTOR = 1e-4, 1.25e-5, 8.0
DEV = "cuda:0"


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


def bar_of(g, k):
    dev = float(g["fp32_dev_" + k])
    return FACTOR * dev if dev > GUARD else BAR


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"dfnet_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def packed_of(name):
    from nerf_loc_amd import _cnn_lib
    _, w = dc.build(name)
    return _cnn_lib.pack_weights([torch.from_numpy(w[n]).to(DEV) for n in _cnn_lib.weight_names()])


@functools.lru_cache(maxsize=None)
def library_run(name):
    """(out, x1, x2, x3) of one library call on the recipe, as device tensors; computed once and shared."""
    from nerf_loc_amd import _cnn_lib
    x, _ = dc.build(name)
    res = _cnn_lib.dfnet_forward(packed_of(name), torch.from_numpy(x).to(DEV), taps=True)
    torch.cuda.synchronize()
    return res


def build_module(name, hip):
    from nerf_loc_amd.depth_fusion import DepthFusionNet
    _, w = dc.build(name)
    m = DepthFusionNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.hip_encode = hip
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", [n for n in dc.CASES if n != "const"])
def test_forward_matches_the_reference_fixture(name):
    g = golden(name)
    errs = {}
    for k, t in zip(dc.TENSORS, library_run(name)):
        got = t.cpu().numpy()
        assert np.isfinite(got).all()
        errs[k] = (rel(got, g[k]), bar_of(g, k))   # every element compared
        print(name, k, "err %.3g bar %.3g recorded fp32_dev %.3g" % (errs[k][0], errs[k][1], float(g["fp32_dev_" + k])))
    assert all(e <= b for e, b in errs.values()), (name, errs)


def test_constant_input_is_finite_and_right_where_the_reference_is_well_conditioned():
    """`const`: every input plane has zero variance, so does every plane of conv1's output, and InstanceNorm multiplies any fp32 rounding there by
    1 / sqrt(eps) = 316.  The fixture records the reference's own fp32 error: 2.4 on `out`, 2.6e-5 on x1, 1.7e-5 on x3 — those three are excluded (above 1.25e-5);
    x2 (1.1e-5) is held to the fp64 fixture."""
    g = golden("const")
    held = [k for k in dc.TENSORS if float(g["fp32_dev_" + k]) <= GUARD]
    assert held == ["x2"]
    for k, t in zip(dc.TENSORS, library_run("const")):
        got = t.cpu().numpy()
        assert np.isfinite(got).all(), k
        print("const", k, "err %.3g recorded fp32_dev %.3g" % (rel(got, g[k]), float(g["fp32_dev_" + k])))
        if k in held:
            assert rel(got, g[k]) <= BAR, k


def test_forward_matches_the_restated_header_at_a_further_shape():
    from nerf_loc_amd import _cnn_lib
    x = dc.make_input(2, 64, 112, 41)
    w = dc.make_weights(41)
    want = dr.dfnet_forward(x, w)
    packed = _cnn_lib.pack_weights([torch.from_numpy(w[n]).to(DEV) for n in _cnn_lib.weight_names()])
    res = _cnn_lib.dfnet_forward(packed, torch.from_numpy(x).to(DEV), taps=True)
    errs = {k: rel(t.cpu().numpy(), want[k]) for k, t in zip(dc.TENSORS, res)}
    print("64x112", errs)
    assert max(errs.values()) <= BAR, errs


def test_two_calls_give_the_same_bits_and_taps_do_not_change_out():
    from nerf_loc_amd import _cnn_lib
    x, _ = dc.build("odd5")
    xd = torch.from_numpy(x).to(DEV)
    first = library_run("odd5")
    again = _cnn_lib.dfnet_forward(packed_of("odd5"), xd, taps=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert torch.equal(_cnn_lib.dfnet_forward(packed_of("odd5"), xd), first[0])   # taps == NULL
    # some taps NULL: the struct with one member set
    lib = _cnn_lib.load()
    V, H, W = x.shape[0], x.shape[2], x.shape[3]
    out, x2 = torch.empty_like(first[0]), torch.empty_like(first[2])
    ws = torch.empty(lib.nlc_dfnet_workspace_bytes(V, H, W), dtype=torch.uint8, device=DEV)
    tp = _cnn_lib.NlcDfnetTaps(None, x2.data_ptr(), None)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.nlc_dfnet_forward(packed_of("odd5").data_ptr(), xd.data_ptr(), V, H, W, out.data_ptr(), ct.byref(tp), ws.data_ptr(), ws.numel(), st) == 0
    assert torch.equal(out, first[0]) and torch.equal(x2, first[2])


def test_a_view_alone_has_the_bits_of_its_slice():
    from nerf_loc_amd import _cnn_lib
    x, _ = dc.build("odd5")
    xd = torch.from_numpy(x).to(DEV)
    full = library_run("odd5")
    for v in range(x.shape[0]):
        alone = _cnn_lib.dfnet_forward(packed_of("odd5"), xd[v:v + 1].contiguous(), taps=True)
        for a, b in zip(alone, full):
            assert torch.equal(a[0], b[v]), v


def test_refused_calls_return_the_documented_codes_and_write_nothing():
    from nerf_loc_amd import _cnn_lib, _lib
    lib = _cnn_lib.load()
    packed = packed_of("min32")
    x = torch.from_numpy(dc.make_input(1, 48, 64, 5)).to(DEV)
    need = lib.nlc_dfnet_workspace_bytes(1, 32, 32)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 32, 12, 16), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda V, H, W, wsp, n: lib.nlc_dfnet_forward(packed.data_ptr(), x.data_ptr(), V, H, W, out.data_ptr(), None, wsp, n, st)
    assert ws.data_ptr() % 256 == 0
    assert call(1, 32, 32, ws.data_ptr(), need - 1) == _lib.NL_ERR_WORKSPACE        # short
    assert call(1, 32, 32, ws.data_ptr() + 16, need) == _lib.NL_ERR_WORKSPACE       # misaligned
    assert call(1, 32, 32, None, need) == _lib.NL_ERR_WORKSPACE
    assert call(1, 40, 64, ws.data_ptr(), need + 256) == _lib.NL_ERR_UNSUPPORTED    # H = 40
    assert call(0, 32, 32, ws.data_ptr(), need) == _lib.NL_ERR_UNSUPPORTED          # V = 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0).all())
    with pytest.raises(ValueError):
        _cnn_lib.dfnet_forward(packed, x[:, :, :40].contiguous())


# ------------------------------------------------------------------------------------------ the module
def test_encode_with_the_switch_matches_eager_and_packs_once():
    x, _ = dc.build("odd5")
    xd = torch.from_numpy(x).to(DEV)
    eager, hip = build_module("odd5", False), build_module("odd5", True)
    g = golden("odd5")
    with torch.no_grad():
        want, got = eager.encode(xd), hip.encode(xd)
        assert got.shape == want.shape and got.is_contiguous()
        print("encode: library vs eager %.3g, eager vs fixture %.3g, library vs fixture %.3g" % (rel(got.cpu(), want.cpu()), rel(want.cpu(), g["out"]), rel(got.cpu(), g["out"])))
        assert rel(got.cpu(), want.cpu()) <= BAR and rel(got.cpu(), g["out"]) <= bar_of(g, "out")
        assert torch.equal(got, library_run("odd5")[0])
        assert torch.equal(hip.encode(xd), got) and hip.pack_count == 1
        hip.fuse_net.conv1.weight.mul_(1.5)   # in place: the cache sees the version
        eager.fuse_net.conv1.weight.mul_(1.5)
        again = hip.encode(xd)
        assert hip.pack_count == 2 and not torch.equal(again, got) and rel(again.cpu(), eager.encode(xd).cpu()) <= BAR
    assert eager.pack_count == 0
    # a call that wants gradients stays eager: same module, chosen per call
    y = hip.encode(xd)
    assert y.requires_grad and hip.pack_count == 2


def test_graph_replay_with_new_inputs_equals_the_direct_call():
    hip = build_module("wide", True)
    x1 = torch.from_numpy(dc.build("wide")[0]).to(DEV)
    x2 = torch.from_numpy(dc.make_input(2, 32, 48, 99)).to(DEV)
    with torch.no_grad():
        static_in = x1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hip.encode(static_in)   # packs the weights outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = hip.encode(static_in)
        for x in (x2, x1):
            static_in.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, hip.encode(x))
    assert hip.pack_count == 1


@pytest.mark.parametrize("precision", ["fp32"])
def test_a_frame_built_with_hip_frame_cnn_renders_within_the_parity_bar(precision):
    """The `setup` case of tests/test_dropin_module.py (3 views, 32 x 48), end to end with the library's encoder: its bar there is 1e-4 against the reference."""
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    from tests.golden_cases import build_setup_case
    from tests.test_dropin_module import _args
    from tests.util import load_golden, rel_err
    case = build_setup_case("setup")
    cfg, frame, rays = case["cfg"], case["frame"], case["rays"]
    g = load_golden("setup")
    dev = torch.device(DEV)
    net = ConditionalNeRF(_args(cfg), precision=precision, hip_frame_cnn=True).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in case["weights"].items()}, strict=True)
    data = {k: torch.from_numpy(frame[k]).to(dev) for k in ("topk_images", "topk_depths", "topk_Ks", "topk_poses", "feat_fine_src", "feat_coarse_src",
                                                           "depth_range", "K", "pose")}
    data.update({"embedding_a": None, "H": frame["H"], "W": frame["W"], "stride_fine": 4, "stride_coarse": 8})
    rd = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in rays.items()}
    net.support_neural_points = None
    net.multiview_aggregator.vis_featmaps = None
    out = net.render_rays(data, rd)
    df = net.multiview_aggregator.depth_fusion
    assert df.hip_encode and df.pack_count == 1   # the library built the maps
    err_cnn = rel_err(net.multiview_aggregator.vis_featmaps.cpu().numpy(), g["vis_featmaps"])
    errs = {k: rel_err(out[k].cpu().numpy(), g[k]) for k in ("rgb", "depth", "weights", "depth_uncertainty", "feat")}
    print("vis_featmaps", err_cnn, errs)
    assert err_cnn <= BAR and max(errs.values()) < 1e-4, (err_cnn, errs)
    assert np.array_equal(out["mask"].cpu().numpy(), g["mask"])
