"""The 2-D backbone of libnerfloc_backbone.so on the GPU: nlb_backbone_forward against the reference's fp64 fixtures (tests/golden/backbone_*.npz) and against the
fp64 restatement of its header, its determinism and view independence, its layouts, its refusals, graph replay, and the opt-in path of Backbone.

The bar for every tensor of every recipe is the project's: max |err| / max |ref| <= 1e-4, every element compared.  There is no relaxed bar: the generator
refuses a recipe on which the reference's own fp32 run misses its fp64 run by more than 1.25e-5 on any tensor.  Both precisions of the library, `"fp32"` and
`"bf16x3"`, are held to that bar on the same fixtures."""
import ctypes as ct
import functools
import os

import numpy as np
import pytest
import torch

from tests import backbone_cases as bc
from tests import backbone_ref as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
DEV = "cuda:0"
OUTS = ("conv1", "layer1", "layer2")
PRECISIONS = ("fp32", "bf16x3")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def golden(name):
    return bc.load_golden(ROOT, name)


@functools.lru_cache(maxsize=None)
def packed_of(name):
    from nerf_loc_amd import _backbone_lib
    _, w, fpn_dim = bc.build(name)
    return _backbone_lib.pack_weights([torch.from_numpy(w[n]).to(DEV) for n in _backbone_lib.weight_names()], fpn_dim)


@functools.lru_cache(maxsize=None)
def images_of(name):
    return torch.from_numpy(bc.build(name)[0]).to(DEV)


@functools.lru_cache(maxsize=None)
def library_run(name, layout="channels_last", precision="fp32"):
    """(conv1, layer1, layer2, tap_layer1, tap_layer2) of one library call on the recipe, as device tensors; computed once and shared."""
    from nerf_loc_amd import _backbone_lib
    res = _backbone_lib.backbone_forward(packed_of(name), images_of(name), bc.CASES[name][3], precision=precision, layout=layout, taps=True)
    torch.cuda.synchronize()
    return res


def build_module(name, hip):
    from nerf_loc_amd.backbone2d import Backbone
    _, w, fpn_dim = bc.build(name)
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=fpn_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.hip_forward = hip
    return m.to(DEV).eval()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(bc.CASES))
def test_forward_matches_the_reference_fixture(name, precision):
    g = golden(name)
    errs = {}
    for k, t in zip(bc.TENSORS, library_run(name, precision=precision)):
        got = t.cpu().numpy()
        assert np.isfinite(got).all(), k
        if k in g:   # the larger cases carry no taps; those are held to the restatement below
            errs[k] = rel(got, g[k])   # every element compared
            print(name, precision, k, "err %.3g recorded fp32_dev %.3g" % (errs[k], float(g["fp32_dev_" + k])))
    assert set(OUTS) <= set(errs) and set(errs) == set(bc.tensors_of(name))
    assert all(e <= BAR for e in errs.values()), (name, errs)


def test_forward_matches_the_restated_header_at_a_further_shape():
    from nerf_loc_amd import _backbone_lib
    imgs, w = bc.make_images(2, 40, 72, 61), bc.make_weights(61, 192)
    want = br.backbone_forward(imgs, w)
    packed = _backbone_lib.pack_weights([torch.from_numpy(w[n]).to(DEV) for n in _backbone_lib.weight_names()], 192)
    res = _backbone_lib.backbone_forward(packed, torch.from_numpy(imgs).to(DEV), 192, taps=True)
    errs = {k: rel(t.cpu().numpy(), want[k]) for k, t in zip(bc.TENSORS, res)}
    print("2x40x72", errs)
    assert max(errs.values()) <= BAR, errs


@functools.lru_cache(maxsize=None)
def restated(name):
    imgs, w, _ = bc.build(name)
    return br.backbone_forward(imgs, w)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["wide", "tiles"])
def test_taps_of_the_larger_cases_match_the_restated_header(name, precision):
    want = restated(name)
    errs = {k: rel(t.cpu().numpy(), want[k]) for k, t in zip(bc.TENSORS, library_run(name, precision=precision))}
    print(name, precision, errs)
    assert max(errs.values()) <= BAR, errs


def test_split_bf16_is_deterministic_view_independent_and_differs_from_fp32():
    from nerf_loc_amd import _backbone_lib
    first = library_run("odd", precision="bf16x3")
    again = _backbone_lib.backbone_forward(packed_of("odd"), images_of("odd"), 192, precision="bf16x3", taps=True)
    alone = _backbone_lib.backbone_forward(packed_of("odd"), images_of("odd")[1:2].contiguous(), 192, precision="bf16x3", taps=True)
    for a, b, c in zip(first, again, alone):
        assert torch.equal(a, b) and torch.equal(c[0], a[1])
    fp32 = library_run("odd")
    assert torch.equal(first[0], fp32[0]) and not torch.equal(first[3], fp32[3])   # conv1 stays fp32; the bottlenecks took the other kernel


def test_two_calls_give_the_same_bits_and_taps_do_not_change_the_outputs():
    from nerf_loc_amd import _backbone_lib
    first = library_run("odd")
    again = _backbone_lib.backbone_forward(packed_of("odd"), images_of("odd"), 192, taps=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for a, b in zip(first, _backbone_lib.backbone_forward(packed_of("odd"), images_of("odd"), 192)):   # taps == NULL
        assert torch.equal(a, b)
    # one tap NULL: the struct with one member set
    lib = _backbone_lib.load()
    x = images_of("odd")
    V, H, W = x.shape[0], x.shape[2], x.shape[3]
    c1, p1, p2, t2 = (torch.empty_like(first[0]), torch.empty(first[1].permute(0, 2, 3, 1).shape, device=DEV), torch.empty(first[2].permute(0, 2, 3, 1).shape, device=DEV),
                      torch.empty_like(first[4]))
    ws = torch.empty(lib.nlb_backbone_workspace_bytes(V, H, W, 192), dtype=torch.uint8, device=DEV)
    tp = _backbone_lib.NlbBackboneTaps(None, t2.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.nlb_backbone_forward(packed_of("odd").data_ptr(), x.data_ptr(), V, H, W, 192, 0, 1, c1.data_ptr(), p1.data_ptr(), p2.data_ptr(), ct.byref(tp),
                                    ws.data_ptr(), ws.numel(), st) == 0
    assert torch.equal(c1, first[0]) and torch.equal(p1.permute(0, 3, 1, 2), first[1]) and torch.equal(p2.permute(0, 3, 1, 2), first[2]) and torch.equal(t2, first[4])


def test_a_view_alone_has_the_bits_of_its_slice():
    from nerf_loc_amd import _backbone_lib
    x = torch.cat([images_of("odd"), torch.from_numpy(bc.make_images(1, 34, 50, 77)).to(DEV)])   # three views
    full = _backbone_lib.backbone_forward(packed_of("odd"), x, 192, taps=True)
    alone = _backbone_lib.backbone_forward(packed_of("odd"), x[1:2].contiguous(), 192, taps=True)
    for a, b in zip(alone, full):
        assert torch.equal(a[0], b[1])
    for a, b in zip(library_run("odd"), full):   # and views 0, 1 of the three-view call are the two-view call
        assert torch.equal(a, b[:2])


@pytest.mark.parametrize("name", ["odd", "min16"])
def test_both_layouts_hold_the_same_values(name):
    nhwc, nchw = library_run(name), library_run(name, "nchw")
    for a, b in zip(nhwc, nchw):
        assert a.shape == b.shape and torch.equal(a, b)
    for i in (1, 2):
        assert nhwc[i].permute(0, 2, 3, 1).is_contiguous() and not nhwc[i].is_contiguous()
        assert nchw[i].is_contiguous()
    assert nhwc[0].is_contiguous() and nhwc[3].is_contiguous() and nhwc[4].is_contiguous()   # conv1 and the taps are NCHW in both


def test_refused_calls_return_the_documented_codes_and_write_nothing():
    from nerf_loc_amd import _backbone_lib, _lib
    lib = _backbone_lib.load()
    packed = packed_of("min16")
    x = torch.from_numpy(bc.make_images(1, 24, 32, 5)).to(DEV)
    need = lib.nlb_backbone_workspace_bytes(1, 16, 16, 64)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    outs = [torch.full((1, 64, 12, 16), 7.0, device=DEV), torch.full((1, 6, 8, 64), 7.0, device=DEV), torch.full((1, 3, 4, 64), 7.0, device=DEV)]
    st = torch.cuda.current_stream().cuda_stream

    def call(V, H, W, fd, prec, lay, wsp, n, packed_ptr=packed.data_ptr()):
        return lib.nlb_backbone_forward(packed_ptr, x.data_ptr(), V, H, W, fd, prec, lay, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, wsp, n, st)
    assert ws.data_ptr() % 256 == 0
    assert call(1, 16, 16, 64, 0, 1, ws.data_ptr(), need - 1) == _lib.NL_ERR_WORKSPACE        # short
    assert call(1, 16, 16, 64, 0, 1, ws.data_ptr() + 16, need) == _lib.NL_ERR_WORKSPACE       # misaligned
    assert call(1, 16, 16, 64, 0, 1, None, need) == _lib.NL_ERR_WORKSPACE
    assert call(1, 15, 16, 64, 0, 1, ws.data_ptr(), need + 256) == _lib.NL_ERR_UNSUPPORTED    # H = 15
    assert call(0, 16, 16, 64, 0, 1, ws.data_ptr(), need) == _lib.NL_ERR_UNSUPPORTED          # V = 0
    assert call(1, 16, 16, 96, 0, 1, ws.data_ptr(), need) == _lib.NL_ERR_UNSUPPORTED          # fpn_dim
    assert call(1, 16, 16, 64, 1, 1, ws.data_ptr(), need - 1) == _lib.NL_ERR_WORKSPACE        # "bf16x3": the same refusals
    assert call(1, 16, 16, 64, 5, 1, ws.data_ptr(), need) == _lib.NL_ERR_BAD_ARG and call(1, 16, 16, 64, 0, 3, ws.data_ptr(), need) == _lib.NL_ERR_BAD_ARG
    assert call(1, 16, 16, 64, 0, 1, ws.data_ptr(), need, packed.data_ptr() + 64) == _lib.NL_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((ws == 0).all())
    with pytest.raises(ValueError):
        _backbone_lib.backbone_forward(packed, x[:, :, :15].contiguous(), 64)
    with pytest.raises(ValueError):
        _backbone_lib.backbone_forward(packed, x, 64, precision="fp16")


def test_graph_replay_with_new_images_equals_the_direct_call():
    hip = build_module("odd", True)
    x1 = images_of("odd")
    x2 = torch.from_numpy(bc.make_images(2, 34, 50, 99)).to(DEV)
    with torch.no_grad():
        static_in = x1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hip(static_in)   # packs the weights outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = hip(static_in)
        for x in (x2, x1):
            static_in.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            direct = hip(x)
            assert all(torch.equal(static_out[k], direct[k]) for k in OUTS)
    assert hip.pack_count == 1


# ------------------------------------------------------------------------------------------ the module
def test_module_path_selection(monkeypatch):
    from nerf_loc_amd import _backbone_lib
    from nerf_loc_amd.backbone2d import Backbone
    calls = []
    real = _backbone_lib.backbone_forward
    monkeypatch.setattr(_backbone_lib, "backbone_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = images_of("odd")
    eager, off, hip = build_module("odd", False), build_module("odd", False), build_module("odd", True)
    g = golden("odd")
    with torch.no_grad():
        want, same, got = eager(x), off(x), hip(x)
        assert not calls[1:] and len(calls) == 1                                   # only the module with the switch took the library
        assert all(torch.equal(same[k], want[k]) for k in OUTS)                    # the switch off: bit-equal to eager
        assert list(got) == list(want) == list(OUTS)
        for k, t in zip(OUTS, library_run("odd")):
            assert torch.equal(got[k], t) and got[k].shape == want[k].shape
            print(k, "library vs eager %.3g, eager vs fixture %.3g, library vs fixture %.3g" % (rel(got[k].cpu(), want[k].cpu()), rel(want[k].cpu(), g[k]), rel(got[k].cpu(), g[k])))
            assert rel(got[k].cpu(), g[k]) <= BAR
        assert got["layer1"].permute(0, 2, 3, 1).is_contiguous() and got["conv1"].is_contiguous()
        hip.hip_output_layout = "nchw"
        assert hip(x)["layer1"].is_contiguous() and torch.equal(hip(x)["layer1"], got["layer1"]) and len(calls) == 3
        hip.hip_precision = "bf16x3"
        b3 = hip(x)
        assert len(calls) == 4 and not torch.equal(b3["layer1"], got["layer1"]) and max(rel(b3[k].cpu(), g[k]) for k in OUTS) <= BAR and hip.pack_count == 1
        hip.hip_precision = "fp32"
        hip.train()                                                                # the mode does not enter the choice
        assert torch.equal(hip(x)["layer2"], got["layer2"]) and len(calls) == 5
    # grad enabled with a trainable layer2: eager, with gradients
    y = hip(x)
    assert len(calls) == 5 and y["layer2"].requires_grad and y["layer1"].requires_grad and not y["conv1"].requires_grad
    (y["layer1"].sum() + y["layer2"].sum()).backward()
    assert hip.body["layer2"][0].conv1.weight.grad is not None and hip.fpn.layer_blocks[0][0].weight.grad is not None
    assert hip.body["layer1"][0].conv1.weight.grad is None   # frozen
    # other configurations: eager
    with torch.no_grad():
        for kw in (dict(return_layers=["conv1", "layer1", "layer2"], use_fpn=False), dict(return_layers=["layer1", "layer2"], use_fpn=True, fpn_dim=64),
                   dict(return_layers=["conv1", "layer1", "layer2", "layer3"], use_fpn=True, fpn_dim=64), dict(return_layers=["conv1", "layer1", "layer2"], use_fpn=True, fpn_dim=96)):
            m = Backbone(**kw).to(DEV)
            m.hip_forward = True
            out = m(x)
            assert list(out) == kw["return_layers"] and m.pack_count == 0
        assert hip.to(torch.float64)(x.double())["layer1"].dtype == torch.float64   # another dtype
    assert len(calls) == 5


def test_pack_count_follows_in_place_changes():
    x = images_of("sq32")
    hip, eager = build_module("sq32", True), build_module("sq32", False)
    with torch.no_grad():
        first = hip(x)
        assert hip.pack_count == 1
        hip(x)
        assert hip.pack_count == 1
        hip.body["layer1"][1].bn2.running_var.mul_(1.5)   # a BN buffer, in place: the cache sees the version
        eager.body["layer1"][1].bn2.running_var.mul_(1.5)
        second = hip(x)
        assert hip.pack_count == 2 and not torch.equal(second["layer1"], first["layer1"]) and torch.equal(second["conv1"], first["conv1"])
        hip.body["layer2"][2].conv2.weight.mul_(0.5)     # a weight
        eager.body["layer2"][2].conv2.weight.mul_(0.5)
        third = hip(x)
        assert hip.pack_count == 3 and not torch.equal(third["layer2"], second["layer2"])
        hip(x)
        assert hip.pack_count == 3
        want = eager(x)
        errs = {k: rel(third[k].cpu(), want[k].cpu()) for k in OUTS}
        print(errs)
        assert max(errs.values()) <= BAR
    assert eager.pack_count == 0
