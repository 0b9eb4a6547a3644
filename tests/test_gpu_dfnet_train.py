"""DepthFusionNet training in libnerfloc_cnn_train.so on the GPU: the kept forward against nlc_dfnet_forward (bits), the 72 gradients against the reference's fp64
fixtures and against the in-repo eager module's fp64 autograd on the CPU (which tests/test_dfnet_train_cpu.py holds to those fixtures at 1e-10), the stage entry
points against the fp64 restatement tests/dfnet_train_ref.py, determinism, NULL gradients, graph replay, refusals, and the module's switch.

The bar per tensor is the rule of tests/test_gpu_dfnet.py: max |err| / max |ref| <= 1e-4; where the truth's OWN fp32 run misses its fp64 run by more than 1.25e-5 on a
tensor, 8 x that deviation.  The deviation is read from the fixture, or computed from the eager module's fp32 CPU run — never from the code under test."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

from tests import dfnet_cases as dc
from tests import dfnet_train_cases as tc
from tests import dfnet_train_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STAGE_BAR = 1e-4


def names():
    from nerf_loc_amd import _cnn_lib
    return _cnn_lib.weight_names()


def eager_grads(x, w, cot, dtype):
    from nerf_loc_amd.depth_fusion import DepthFusionNet
    m = DepthFusionNet().to(dtype)
    m.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in w.items()}, strict=True)
    (m.encode(torch.from_numpy(x).to(dtype)) * torch.from_numpy(cot).to(dtype)).sum().backward()
    return {k: p.grad.double().numpy() for k, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def truth(name):
    """({tensor: fp64 gradient}, {tensor: fp32_dev}) of the in-repo eager module on the CPU; computed once and shared, never written to."""
    x, w, cot = tc.build(name)
    g64, g32 = eager_grads(x, w, cot, torch.float64), eager_grads(x, w, cot, torch.float32)
    dev = {k: 0.0 if k in tc.ZERO_BIASES else float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64}
    return g64, dev


@functools.lru_cache(maxsize=None)
def library_run(name):
    """(packed, cnn_in, out, state, g_out, grads, state0) of one forward + backward of the library on a SWEEP entry; computed once and shared.  The state starts
    as zeros (the padding between its buffers is never written); state0 is its copy taken between the two calls."""
    from nerf_loc_amd import _cnn_train_lib as T
    x, w, cot = tc.build(name)
    ts = [torch.from_numpy(w[n]).to(DEV) for n in names()]
    xd, g_out = torch.from_numpy(x).to(DEV), torch.from_numpy(cot).float().to(DEV)
    packed = T.pack_weights(ts)
    V, H, W = x.shape[0], x.shape[2], x.shape[3]
    out, state = T.dfnet_forward_train(packed, xd, state=torch.zeros(T.load().nlct_dfnet_state_bytes(V, H, W), dtype=torch.uint8, device=DEV))
    state0 = state.clone()
    grads = T.dfnet_backward(packed, xd, state, g_out, [tuple(t.shape) for t in ts])
    torch.cuda.synchronize()
    return packed, xd, out, state, g_out, grads, state0


def check_grads(tag, got, ref, dev):
    """got {name: array}; every tensor under the bar rule, the four cancelled biases exact zeros; prints error and bar per tensor."""
    worst, bad = (0.0, "", 0.0), []
    for k in names():
        a = np.asarray(got[k])
        assert np.isfinite(a).all(), k
        if k in tc.ZERO_BIASES:
            assert not a.any(), (tag, k, "must be exact zeros")
            continue
        e, b = tc.rel(a, ref[k]), tc.bar_of(dev[k])
        print("%s %-44s err %.3g bar %.3g fp32_dev %.3g" % (tag, k, e, b, dev[k]))
        worst = max(worst, (e / b, k, e))
        if e > b:
            bad.append((k, e, b))
    print("%s worst: %s err %.3g (%.2f of its bar)" % (tag, worst[1], worst[2], worst[0]))
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(tc.SWEEP))
def test_forward_train_has_the_bits_of_the_inference_forward_and_keeps_its_state(name):
    from nerf_loc_amd import _cnn_lib, _cnn_train_lib as T
    packed, xd, out, state, g_out, _, state0 = library_run(name)
    _, w, _ = tc.build(name)
    ref = _cnn_lib.dfnet_forward(_cnn_lib.pack_weights([torch.from_numpy(w[n]).to(DEV) for n in names()]), xd, taps=True)
    assert torch.equal(out, ref[0])
    assert torch.equal(_cnn_lib.dfnet_forward(packed, xd), ref[0])     # the training image begins with the inference image
    out2, state2 = T.dfnet_forward_train(packed, xd, state=torch.zeros_like(state))
    assert torch.equal(out2, out) and torch.equal(state2, state0)
    assert torch.equal(state, state0)                                   # the backward left the state as the forward wrote it
    # x1, x2, x3 lie in the state with the inference forward's bits
    flat = state.view(torch.float32)
    for t in ref[1:]:
        n, first = t.numel(), t.flatten()[:64]
        hits = (flat.unfold(0, 64, 64) == first).all(dim=1).nonzero().flatten().tolist()   # every buffer starts at a multiple of 64 values
        assert any(torch.equal(flat[64 * h:64 * h + n], t.flatten()) for h in hits)


# ------------------------------------------------------------------------------------------ the 72 gradients
@pytest.mark.parametrize("name", tc.RECIPES)
def test_gradients_meet_the_reference_fixture(name):
    assert tc.SWEEP[name] == dc.CASES[name]
    g = tc.fixture(name)
    got = {k: t.cpu().numpy() for k, t in zip(names(), library_run(name)[5])}
    check_grads("fixture " + name, got, {k: g["grad_" + k] for k in names()}, {k: float(g["fp32_dev_" + k]) for k in names()})


@pytest.mark.parametrize("name", list(tc.SWEEP))
def test_gradients_meet_the_eager_fp64_truth(name):
    ref, dev = truth(name)
    got = {k: t.cpu().numpy() for k, t in zip(names(), library_run(name)[5])}
    check_grads("truth " + name, got, ref, dev)


# ------------------------------------------------------------------------------------------ the stages
CONV_CASES = [  # ks, stride, hin, win, C0, C1, cout, data gradient
    (3, 1, 2, 2, 32, 32, 32, True), (3, 1, 3, 5, 64, 0, 32, True), (3, 2, 5, 5, 32, 0, 64, True), (3, 2, 23, 39, 32, 0, 32, True), (3, 1, 16, 24, 32, 32, 32, True),
    (3, 2, 2, 2, 32, 0, 32, True), (3, 2, 3, 3, 32, 32, 32, True), (1, 2, 23, 39, 32, 0, 32, True), (1, 2, 2, 2, 32, 0, 64, True), (1, 2, 3, 5, 32, 32, 32, True),
    (1, 2, 16, 24, 64, 0, 32, True), (8, 2, 16, 24, 12, 0, 32, False), (8, 2, 5, 23, 12, 0, 32, False),
]


@pytest.mark.parametrize("ks,stride,hin,win,C0,C1,cout,dgrad", CONV_CASES)
def test_conv_backward_stage(ks, stride, hin, win, C0, C1, cout, dgrad):
    from nerf_loc_amd import _cnn_train_lib as T
    rng = np.random.default_rng(1000 * ks + 100 * stride + hin + win)
    V, pad = 2, tr.PAD[ks]
    ho, wo = (hin + 2 * pad - ks) // stride + 1, (win + 2 * pad - ks) // stride + 1
    x = rng.standard_normal((V, C0 + C1, hin, win)).astype(np.float32)
    w = (rng.standard_normal((cout, C0 + C1, ks, ks)) / np.sqrt((C0 + C1) * ks * ks)).astype(np.float32)
    g = rng.standard_normal((V, cout, ho, wo)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    g_x0, g_x1, g_w = T.conv_backward(t(x[:, :C0]), t(x[:, C0:]) if C1 else None, t(w), t(g), stride, want_x=dgrad)
    ref_x, ref_w = tr.conv_backward(x, w, g, stride)
    e_w = tc.rel(g_w.cpu().numpy(), ref_w)
    print("conv k%d s%d %dx%d (%d+%d)->%d  g_w err %.3g" % (ks, stride, hin, win, C0, C1, cout, e_w))
    assert e_w <= STAGE_BAR
    if dgrad:
        got = np.concatenate([g_x0.cpu().numpy()] + ([g_x1.cpu().numpy()] if C1 else []), axis=1)
        e_x = tc.rel(got, ref_x)
        print("    g_x err %.3g" % e_x)
        assert e_x <= STAGE_BAR
        # each output alone has the same bits
        only_w = T.conv_backward(t(x[:, :C0]), t(x[:, C0:]) if C1 else None, t(w), t(g), stride, want_x=False)[2]
        only_x = T.conv_backward(t(x[:, :C0]), t(x[:, C0:]) if C1 else None, t(w), t(g), stride, want_w=False)[0]
        assert torch.equal(only_w, g_w) and torch.equal(only_x, g_x0)


@pytest.mark.parametrize("n", [4, 15, 897])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_instnorm_backward_stage(n, act):
    from nerf_loc_amd import _cnn_train_lib as T
    rng = np.random.default_rng(n + act)
    V, C = 3, 5
    x = rng.standard_normal((V, C, n)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 2, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    nrm = tr.make_norm(x, gamma, beta)
    y = tr.act_of(x, nrm, act).astype(np.float32)
    g = rng.standard_normal((V, C, n)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    xd, nd, yd = t(x), t(nrm), t(y)
    got = T.instnorm_backward(xd, nd, None if act == 0 else yd, act, t(g))
    ref = tr.instnorm_backward(x, nrm, y, act, g)
    errs = [tc.rel(a.cpu().numpy(), b) for a, b in zip(got, ref)]
    print("instnorm n %d act %d: g_x %.3g g_gamma %.3g g_beta %.3g" % (n, act, *errs))
    assert max(errs) <= STAGE_BAR
    gi = t(g).clone()   # in place: g_x may be g_y itself
    lib, ws = T.load(), torch.empty(8 * V * C + 256, dtype=torch.uint8, device=DEV)
    assert lib.nlct_instnorm_backward(xd.data_ptr(), nd.data_ptr(), None if act == 0 else yd.data_ptr(), act, gi.data_ptr(), V, C, n, gi.data_ptr(), None, None,
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(gi, got[0])


@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (8, 12)])
def test_up2_backward_stage(h, w):
    from nerf_loc_amd import _cnn_train_lib as T
    g = np.random.default_rng(h * w).standard_normal((3, 2 * h, 2 * w)).astype(np.float32)
    e = tc.rel(T.up2_backward(torch.from_numpy(g).to(DEV)).cpu().numpy(), tr.up2_backward(g))
    print("up2 backward from %dx%d: %.3g" % (h, w, e))
    assert e <= STAGE_BAR


# ------------------------------------------------------------------------------------------ properties
def test_two_backward_calls_give_the_same_bits_and_a_null_entry_changes_no_other():
    from nerf_loc_amd import _cnn_train_lib as T
    packed, xd, out, state, g_out, grads, _ = library_run("odd5")
    shapes = [tuple(g.shape) for g in grads]
    again = T.dfnet_backward(packed, xd, state, g_out, shapes)
    assert all(torch.equal(a, b) for a, b in zip(again, grads))
    nm = names()
    off = {nm.index("fuse_net.layer2.0.conv1.weight"), nm.index("fuse_net.bn1.weight"), nm.index("conv_out.bias"), nm.index("fuse_net.iconv3.conv.bias"),
           nm.index("depth_skip.0.weight")}
    some = T.dfnet_backward(packed, xd, state, g_out, shapes, wanted=[i not in off for i in range(72)])
    for i, (a, b) in enumerate(zip(some, grads)):
        assert (a is None) if i in off else torch.equal(a, b), nm[i]


def test_forward_and_backward_replay_bit_for_bit_from_a_graph():
    from nerf_loc_amd import _cnn_train_lib as T
    packed, xd, out, state, g_out, grads, _ = library_run("wide")
    lib = T.load()
    V, H, W = tc.SWEEP["wide"][:3]
    s_in, s_g = xd.clone(), g_out.clone()
    s_out, s_state = torch.empty_like(out), torch.empty_like(state)
    s_ws = torch.empty(lib.nlct_dfnet_backward_workspace_bytes(V, H, W), dtype=torch.uint8, device=DEV)
    s_grads = [torch.empty_like(g) for g in grads]
    ptrs = (ct.c_void_p * 72)(*[g.data_ptr() for g in s_grads])

    def pair():
        st = torch.cuda.current_stream().cuda_stream
        assert lib.nlct_dfnet_forward_train(packed.data_ptr(), s_in.data_ptr(), V, H, W, s_out.data_ptr(), s_state.data_ptr(), s_state.numel(), st) == 0
        assert lib.nlct_dfnet_backward(packed.data_ptr(), s_in.data_ptr(), V, H, W, s_state.data_ptr(), s_g.data_ptr(), ptrs, s_ws.data_ptr(), s_ws.numel(), st) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair()
    x2 = torch.from_numpy(dc.make_input(V, H, W, 99)).to(DEV)
    out2, state2 = T.dfnet_forward_train(packed, x2)
    grads2 = T.dfnet_backward(packed, x2, state2, g_out, [tuple(g.shape) for g in grads])
    for x, o, gs in ((x2, out2, grads2), (xd, out, grads)):
        s_in.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_out, o) and all(torch.equal(a, b) for a, b in zip(s_grads, gs))


def test_refused_calls_return_the_documented_codes_and_write_nothing():
    from nerf_loc_amd import _cnn_train_lib as T, _lib
    lib = T.load()
    packed, xd, out, state, g_out, grads, _ = library_run("min32")
    sb, wb = lib.nlct_dfnet_state_bytes(1, 32, 32), lib.nlct_dfnet_backward_workspace_bytes(1, 32, 32)
    assert sb == state.numel()
    st_buf = torch.zeros(sb + 256, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(wb + 256, dtype=torch.uint8, device=DEV)
    o = torch.full_like(out, 7.0)
    gs = [torch.full_like(g, 7.0) for g in grads]
    ptrs = (ct.c_void_p * 72)(*[g.data_ptr() for g in gs])
    st = torch.cuda.current_stream().cuda_stream
    fwd = lambda V, H, W, sp, n: lib.nlct_dfnet_forward_train(packed.data_ptr(), xd.data_ptr(), V, H, W, o.data_ptr(), sp, n, st)   # noqa: E731
    assert fwd(1, 32, 32, st_buf.data_ptr(), sb - 1) == _lib.NL_ERR_WORKSPACE and fwd(1, 32, 32, st_buf.data_ptr() + 16, sb) == _lib.NL_ERR_WORKSPACE
    assert fwd(1, 32, 32, None, sb) == _lib.NL_ERR_WORKSPACE and fwd(1, 40, 32, st_buf.data_ptr(), sb + 256) == _lib.NL_ERR_UNSUPPORTED
    assert fwd(0, 32, 32, st_buf.data_ptr(), sb) == _lib.NL_ERR_UNSUPPORTED
    bwd = lambda V, H, W, wp, n: lib.nlct_dfnet_backward(packed.data_ptr(), xd.data_ptr(), V, H, W, state.data_ptr(), g_out.data_ptr(), ptrs, wp, n, st)   # noqa: E731
    assert bwd(1, 32, 32, ws.data_ptr(), wb - 1) == _lib.NL_ERR_WORKSPACE and bwd(1, 32, 32, ws.data_ptr() + 16, wb) == _lib.NL_ERR_WORKSPACE
    assert bwd(1, 32, 32, None, wb) == _lib.NL_ERR_WORKSPACE and bwd(1, 32, 40, ws.data_ptr(), wb + 256) == _lib.NL_ERR_UNSUPPORTED
    assert bwd(65, 32, 32, ws.data_ptr(), wb) == _lib.NL_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((st_buf == 0).all()) and bool((ws == 0).all()) and all(bool((g == 7.0).all()) for g in gs)
    with pytest.raises(ValueError):
        T.dfnet_forward_train(packed, xd[:, :, :24].contiguous())


# ------------------------------------------------------------------------------------------ the module
def build_module(name, training):
    from nerf_loc_amd.depth_fusion import DepthFusionNet
    _, w, _ = tc.build(name)
    m = DepthFusionNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.hip_training = training
    return m.to(DEV).train()


def test_module_gradients_meet_the_truth_and_the_cache_follows_the_parameters():
    x, _, cot = tc.build("odd5")
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cot).float().to(DEV)
    m = build_module("odd5", True)
    y = m.encode(xd)
    assert y.requires_grad and m.pack_count == 1 and torch.equal(y.detach(), library_run("odd5")[2])
    y.mul(cd).sum().backward()
    ref, dev = truth("odd5")
    got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    check_grads("module odd5", got, ref, dev)
    for k, g in zip(names(), library_run("odd5")[5]):
        assert torch.equal(dict(m.named_parameters())[k].grad, g), k     # the node is the library pair, nothing else
    m.encode(xd)
    assert m.pack_count == 1
    with torch.no_grad():
        m.fuse_net.conv1.weight.mul_(1.5)   # what an optimizer step does: in place
    y2 = m.encode(xd)
    assert m.pack_count == 2 and not torch.equal(y2.detach(), y.detach())
    # a second-order backward raises
    y3 = m.encode(xd)
    (g1,) = torch.autograd.grad(y3.mul(cd).sum(), m.conv_out.weight, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_a_frozen_layer_gets_no_gradient_and_the_rest_keep_their_bits():
    x, _, cot = tc.build("wide")
    xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(cot).float().to(DEV)
    full, part = build_module("wide", True), build_module("wide", True)
    for p in part.fuse_net.layer1.parameters():
        p.requires_grad_(False)
    full.encode(xd).mul(cd).sum().backward()
    part.encode(xd).mul(cd).sum().backward()
    for (k, a), (_, b) in zip(full.named_parameters(), part.named_parameters()):
        if k.startswith("fuse_net.layer1."):
            assert b.grad is None and a.grad is not None, k
        else:
            assert torch.equal(a.grad, b.grad), k


def test_with_the_switch_off_or_an_input_that_wants_a_gradient_the_eager_path_is_taken(monkeypatch):
    from nerf_loc_amd import _cnn_train_lib as T
    calls = []
    real = T.dfnet_forward_train
    monkeypatch.setattr(T, "dfnet_forward_train", lambda *a, **k: calls.append(1) or real(*a, **k))
    x, _, cot = tc.build("wide")
    xd = torch.from_numpy(x).to(DEV)
    off, on = build_module("wide", False), build_module("wide", True)
    y = off.encode(xd)
    assert y.requires_grad and not calls and off.pack_count == 0
    on.encode(xd.clone().requires_grad_())         # cnn_in wants a gradient: eager
    assert on._use_hip_training(xd[:, :, :, :40].contiguous()) is False and on._use_hip_training(xd.double()) is False   # outside the limits; another dtype
    with torch.no_grad():
        on.encode(xd)                              # no gradient wanted
    for p in on.parameters():
        p.requires_grad_(False)
    on.encode(xd)                                  # no parameter wants one
    assert not calls and on.pack_count == 0
    for p in on.parameters():
        p.requires_grad_(True)
    on.encode(xd)
    assert calls == [1] and on.pack_count == 1


def test_ref_depth_loss_gradients_through_the_library_node_meet_the_fp64_truth():
    """compute_ref_depth_loss reaches only this net (and the mean decoder): the `setup` frame of tests/test_dropin_module.py (3 views, 32 x 48), switch on, against the
    same loss in fp64 on the CPU from the device's cnn_in copied over."""
    from nerf_loc_amd.conditional_nerf import ConditionalNeRF
    from nerf_loc_amd.frame_setup import cross_view_features
    from tests.golden_cases import build_setup_case
    from tests.test_dropin_module import _args
    from tests.util import load_golden
    case = build_setup_case("setup")
    cfg, frame, g = case["cfg"], case["frame"], load_golden("setup")
    t = torch.from_numpy
    near, far = [float(v) for v in frame["depth_range"][0]]
    dev = torch.device(DEV)
    with torch.no_grad():
        cnn_in = cross_view_features(t(frame["topk_images"]).to(dev), t(frame["topk_depths"]).to(dev), t(frame["topk_Ks"]).to(dev), t(frame["topk_poses"]).to(dev),
                                     near, far)

    def grads(dtype, device, training):
        net = ConditionalNeRF(_args(cfg), hip_frame_cnn_training=training).to(dtype).to(device).train()
        net.load_state_dict({k: t(v).to(dtype) for k, v in case["weights"].items()}, strict=True)
        c = lambda a: t(a).to(device=device, dtype=dtype)   # noqa: E731
        agg = net.multiview_aggregator
        agg.vis_featmaps = None
        loss = agg.compute_ref_depth_loss(c(frame["topk_Ks"]), c(frame["topk_poses"]), c(frame["topk_images"]), c(frame["feat_fine_src"]).permute(0, 3, 1, 2),
                                          c(frame["topk_depths"]), c(g["ref_depth_gt"]), c(frame["depth_range"])[0], cnn_in=cnn_in.to(device=device, dtype=dtype))
        loss.backward()
        return float(loss), {k: p.grad.double().cpu().numpy() for k, p in agg.depth_fusion.named_parameters()}, agg.depth_fusion.pack_count
    l64, g64, _ = grads(torch.float64, "cpu", False)
    l32, g32, _ = grads(torch.float32, "cpu", False)
    lg, gg, packs = grads(torch.float32, dev, True)
    assert packs == 1 and abs(lg - l64) <= 1e-4 * abs(l64)
    devs = {k: 0.0 if k in tc.ZERO_BIASES else float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64}
    check_grads("ref_depth_loss", gg, g64, devs)
