"""The sixth library's boundary and the 2-D backbone's contract, without a GPU: header against binding against symbol table, the weight names against the drop-in's
state dict and the reference's recorded key list, the eager drop-in and the header's arithmetic (tests/backbone_ref.py) against the reference's fixtures, the
freezing rule, the nearest-neighbour index rule, and the opt-in switch of Backbone on the CPU."""
import ctypes as ct
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nerf_loc_amd import _app_lib, _backbone_lib, _cabi, _cnn_lib, _geom_lib, _head_lib, _lib
from nerf_loc_amd.backbone2d import Backbone, FrozenBatchNorm2d
from tests import backbone_cases as bc
from tests import backbone_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerfloc_backbone.h")
EXACT = 1e-10     # fp64 programs against the reference's fp64
BAR = 1e-4        # the project's bar: max |err| / max |ref|
GUARD = 1.25e-5   # the generator refuses a recipe whose reference fp32 run misses its fp64 run by more than this on any tensor


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def golden(name):
    return bc.load_golden(ROOT, name)


def build_module(name, dtype=torch.float32):
    _, w, fpn_dim = bc.build(name)
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=fpn_dim)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return m.to(dtype)


def run_with_taps(m, x):
    got = {}
    hooks = [m.body[l].register_forward_hook(lambda mod, a, o, l=l: got.__setitem__("tap_" + l, o.detach().clone())) for l in ("layer1", "layer2")]
    with torch.no_grad():
        got.update(m(x))
    for h in hooks:
        h.remove()
    return {k: v.numpy() for k, v in got.items()}


# ------------------------------------------------------------------------------------------ the sixth library's boundary
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nlb_[a-z_0-9]+)\s*\(", src)))


def _exported(path):
    res = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return sorted(line.split()[-1] for line in res.stdout.splitlines() if line.strip())


def test_backbone_library_header_binding_and_symbol_table_agree():
    assert os.path.exists(_backbone_lib.LIB_PATH), "run __graft_entry__.build() first"
    declared = _declared()
    assert len(declared) == 7 and "nlb_backbone_forward" in declared and "nlb_backbone_pack_weights" in declared
    assert sorted(n for n, _, _ in _backbone_lib.SYMBOLS) == declared
    assert _exported(_backbone_lib.LIB_PATH) == declared   # nothing else: no kernel stubs, no symbol of another library
    lib = _backbone_lib.load()
    hdr = open(HEADER).read()
    assert lib.nlb_abi_version() == _backbone_lib.ABI_VERSION == int(re.search(r"#define\s+NLB_ABI_VERSION\s+(\d+)", hdr).group(1)) == 1
    assert _backbone_lib.NUM_WEIGHTS == 124 and _backbone_lib.LAUNCHES == 35
    assert [lib.nlb_backbone_num_weights(f) for f in (64, 128, 192, 256, 96, 0)] == [124, 124, 124, 124, 0, 0]
    # signatures: read from the header, no hand-written argtypes
    sig = {n: (r, a) for n, r, a in _backbone_lib.SYMBOLS}
    V, I, Z = ct.c_void_p, ct.c_int, ct.c_size_t
    assert sig["nlb_backbone_forward"] == (I, [V, V, I, I, I, I, I, I, V, V, V, ct.POINTER(_backbone_lib.NlbBackboneTaps), V, Z, V])
    assert sig["nlb_backbone_pack_weights"] == (I, [ct.POINTER(V), I, I, V, Z, V])
    assert sig["nlb_backbone_weight_name"] == (ct.c_char_p, [I]) and sig["nlb_backbone_workspace_bytes"] == (Z, [I, I, I, I])
    assert _cabi.struct_fields("nerfloc_backbone.h") == {"nlb_backbone_taps": [("layer1", V), ("layer2", V)]}
    assert ct.sizeof(_backbone_lib.NlbBackboneTaps) == 16
    assert not re.search(r"\.(argtypes|restype)\s*=", open(os.path.join(ROOT, "nerf_loc_amd", "_backbone_lib.py")).read())


def test_the_other_five_libraries_export_no_backbone_symbol():
    for other in (_lib, _head_lib, _app_lib, _geom_lib, _cnn_lib):
        assert not [n for n in _exported(other.LIB_PATH) if n.startswith("nlb_")]


def test_weight_names_are_the_state_dict_keys_and_the_references_key_list():
    names = _backbone_lib.weight_names()   # a host-only query
    assert len(names) == 124 and names[0] == "body.conv1.weight" and names[-1] == "fpn.layer_blocks.1.0.weight"
    lib = _backbone_lib.load()
    assert lib.nlb_backbone_weight_name(-1) is None and lib.nlb_backbone_weight_name(124) is None
    for fpn_dim in (64, 128, 192, 256):
        sd = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=fpn_dim).state_dict()
        assert list(sd.keys()) == names
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == bc.weight_shapes(fpn_dim)
        assert lib.nlb_backbone_packed_bytes(fpn_dim) % 256 == 0 and lib.nlb_backbone_packed_bytes(fpn_dim) > 0
    assert lib.nlb_backbone_packed_bytes(96) == 0
    for name, (_, _, _, fpn_dim, _, _) in bc.CASES.items():
        g = golden(name)
        assert [str(k) for k in g["state_dict_keys"]] == names        # recorded from the reference
        shapes = [tuple(int(d) for d in row if d) for row in g["state_dict_shapes"]]
        assert list(zip(names, shapes)) == bc.weight_shapes(fpn_dim)
        assert "torchvision" in str(g["torchvision_source"])


def test_strict_loading_holds_in_both_directions():
    """The recipe's dict carries exactly the reference's recorded keys: it loads strictly, and the module's own state dict has the same keys and shapes, so a
    reference module would load it strictly too.  A checkpoint's num_batches_tracked is dropped."""
    _, w, fpn_dim = bc.build("sq32")
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=fpn_dim)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert [str(k) for k in golden("sq32")["state_dict_keys"]] == list(m.state_dict().keys())
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "body.bn1.running_var"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{"fpn.inner_blocks.0.1.weight": torch.ones(fpn_dim)}), strict=True)   # the pyramid's InstanceNorm has no parameters
    m.load_state_dict(dict(sd, **{"body.bn1.num_batches_tracked": torch.tensor(3)}), strict=True)
    assert isinstance(m.body["bn1"], FrozenBatchNorm2d) and not list(m.body["bn1"].parameters())
    assert all(c.bias is None for c in m.modules() if isinstance(c, torch.nn.Conv2d))


# ------------------------------------------------------------------------------------------ the arithmetic against the reference
@pytest.mark.parametrize("name", list(bc.CASES))
def test_eager_dropin_equals_the_reference(name):
    imgs, _, fpn_dim = bc.build(name)
    g = golden(name)
    (h1, w1), (h2, w2), (h3, w3) = bc.plane_sizes(*imgs.shape[2:])
    V = imgs.shape[0]
    assert g["conv1"].shape == (V, 64, h1, w1) and g["layer1"].shape == (V, fpn_dim, h2, w2) and g["layer2"].shape == (V, fpn_dim, h3, w3)
    r64 = run_with_taps(build_module(name, torch.float64), torch.from_numpy(imgs).double())
    r32 = run_with_taps(build_module(name), torch.from_numpy(imgs))
    assert list(r64)[-3:] == ["conv1", "layer1", "layer2"]   # an OrderedDict in the ResNet's order
    for k in bc.tensors_of(name):
        e64, e32 = rel(r64[k], g[k]), rel(r32[k], g[k])
        print(name, k, "fp64 %.3g fp32 %.3g recorded fp32_dev %.3g" % (e64, e32, float(g["fp32_dev_" + k])))
        assert g[k].dtype == np.float64 and np.isfinite(r32[k]).all()
        assert e64 <= EXACT and e32 <= BAR, (name, k, e64, e32)
    assert all(0 < float(g["fp32_dev_" + k]) <= GUARD for k in bc.TENSORS)   # all five are recorded, the taps of the larger cases too


@pytest.mark.parametrize("name", list(bc.CASES))
def test_restated_header_equals_the_reference(name):
    """With the image constants as an fp64 program holds them the restatement is the reference's fp64 run; with the header's fp32-rounded constants it is 4e-8
    away, which is what the library is held to on the GPU."""
    imgs, w, _ = bc.build(name)
    g, r, rh = golden(name), br.backbone_forward(imgs, w, fp32_constants=False), br.backbone_forward(imgs, w)
    for k in bc.tensors_of(name):
        print(name, k, rel(r[k], g[k]), rel(rh[k], g[k]))
        assert rel(r[k], g[k]) <= EXACT and rel(rh[k], g[k]) <= 1e-6, (name, k)


def test_every_reference_configuration_runs_eagerly():
    x = torch.rand(1, 3, 32, 40)
    with torch.no_grad():
        m = Backbone(["layer1", "layer2", "layer3", "layer4"])
        y = m(x)
        assert list(y) == ["layer1", "layer2", "layer3", "layer4"] and [v.shape[1] for v in y.values()] == [256, 512, 1024, 2048]
        assert y["layer4"].shape[2:] == (1, 2) and not m.use_fpn and not hasattr(m, "fpn")
        assert m.layer_to_stride == {"conv1": 2, "layer1": 4, "layer2": 8, "layer3": 16, "layer4": 32}
        m = Backbone(["conv1", "layer1", "layer2", "layer3"], use_fpn=True)
        y = m(x)
        assert [tuple(v.shape[1:]) for v in y.values()] == [(64, 16, 20), (128, 8, 10), (128, 4, 5), (128, 2, 3)]
        assert m.layer_to_channels == {"conv1": 64, "layer1": 128, "layer2": 128, "layer3": 128, "layer4": 2048}
        assert len(m.fpn.inner_blocks) == 3 and "layer4" not in m.body and m.return_layers == ["conv1", "layer1", "layer2", "layer3"]
        y = Backbone(["layer2"], use_fpn=True, fpn_dim=32)(x)
        assert list(y) == ["layer2"] and y["layer2"].shape == (1, 32, 4, 5)
    with pytest.raises(ValueError):
        Backbone(["layer5"])


def test_the_module_needs_no_torchvision():
    code = ("import sys; sys.modules['torchvision'] = None\n"   # an import of it now raises ImportError
            "import torch\n"
            "from nerf_loc_amd.backbone2d import Backbone\n"
            "y = Backbone(['conv1', 'layer1', 'layer2'], use_fpn=True, fpn_dim=64)(torch.rand(1, 3, 16, 16))\n"
            "assert [tuple(v.shape) for v in y.values()] == [(1, 64, 8, 8), (1, 64, 4, 4), (1, 64, 2, 2)]\n"
            "assert not [m for m in sys.modules if m.startswith('torchvision.')]\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]


def test_freezing_rule():
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=64)
    for n, p in m.named_parameters():
        assert p.requires_grad == (n.startswith("body.layer2.") or n.startswith("fpn.")), n
    assert any(n.startswith("body.layer2.") for n, _ in m.named_parameters()) and sum(1 for _ in m.fpn.parameters()) == 4
    m = Backbone(["layer1", "layer2", "layer3", "layer4"])
    for n, p in m.named_parameters():
        assert p.requires_grad == (n.split(".")[1] in ("layer2", "layer3", "layer4")), n
    m = Backbone(list(bc.RETURN_LAYERS), train_backbone=False, use_fpn=True)
    assert not any(p.requires_grad for p in m.body.parameters()) and all(p.requires_grad for p in m.fpn.parameters())


# ------------------------------------------------------------------------------------------ limits and refusals
def test_limits_and_refusals_without_a_device():
    lib = _backbone_lib.load()
    buf = (ct.c_char * 8192)()
    p = (ct.addressof(buf) + 255) // 256 * 256   # a HOST address no call below may read: every call here is refused before a launch
    for V, H, W, fd in ((1, 16, 16, 64), (2, 34, 50, 192), (3, 47, 61, 128), (11, 480, 640, 192), (64, 512, 512, 256), (1, 17, 4096, 64)):
        assert lib.nlb_backbone_workspace_bytes(V, H, W, fd) > 0 and _backbone_lib.supported(V, H, W, fd)
    for V, H, W, fd in ((0, 32, 32, 64), (65, 32, 32, 64), (1, 15, 32, 64), (1, 32, 15, 64), (-1, 32, 32, 64), (64, 512, 513, 64), (1, 32, 32, 96), (1, 32, 32, 0),
                        (1, 32, 32, 320)):
        assert lib.nlb_backbone_workspace_bytes(V, H, W, fd) == 0 and not _backbone_lib.supported(V, H, W, fd)
    need = lib.nlb_backbone_workspace_bytes(1, 32, 32, 64)
    FP32, B3, NCHW, NHWC = (_backbone_lib.PRECISIONS["fp32"], _backbone_lib.PRECISIONS["bf16x3"], _backbone_lib.LAYOUTS["nchw"], _backbone_lib.LAYOUTS["channels_last"])

    def call(packed=p, x=p, V=1, H=32, W=32, fd=64, prec=FP32, lay=NHWC, c1=p, p1=p, p2=p, taps=None, ws=p, n=need):
        return lib.nlb_backbone_forward(packed, x, V, H, W, fd, prec, lay, c1, p1, p2, taps, ws, n, None)
    U, B, WS = _lib.NL_ERR_UNSUPPORTED, _lib.NL_ERR_BAD_ARG, _lib.NL_ERR_WORKSPACE
    assert call(H=15, n=1 << 30) == U and call(V=0, n=1 << 30) == U and call(fd=96, n=1 << 30) == U and call(V=65, n=1 << 40) == U
    assert call(prec=B3, H=15) == U and call(prec=B3, ws=None) == WS   # the split-bf16 mode has the same limits
    assert call(prec=7) == B and call(lay=2) == B and call(lay=-1) == B
    assert call(packed=None) == B and call(x=None) == B and call(c1=None) == B and call(p1=None) == B and call(p2=None) == B
    assert call(packed=p + 16) == B and call(x=p + 2) == B and call(c1=p + 1) == B and call(p1=p + 2) == B and call(p2=p + 3) == B
    assert call(taps=ct.byref(_backbone_lib.NlbBackboneTaps(p + 2, None))) == B and call(taps=ct.byref(_backbone_lib.NlbBackboneTaps(None, p + 1))) == B
    assert call(ws=None) == WS and call(n=need - 1) == WS and call(ws=p + 16) == WS and call(lay=NCHW, n=0) == WS
    ptrs = (ct.c_void_p * 124)(*([p] * 124))
    nb = lib.nlb_backbone_packed_bytes(64)
    pack = lib.nlb_backbone_pack_weights
    assert pack(ptrs, 123, 64, p, nb, None) == B and pack(None, 124, 64, p, nb, None) == B and pack(ptrs, 124, 96, p, nb, None) == U
    assert pack(ptrs, 124, 64, p, nb - 1, None) == WS and pack(ptrs, 124, 64, p + 16, nb, None) == WS and pack(ptrs, 124, 64, None, nb, None) == WS
    assert pack(ptrs, 124, 256, p, nb, None) == WS            # a wider pyramid's image is longer
    ptrs[5] = None
    assert pack(ptrs, 124, 64, p, nb, None) == B
    ptrs[5] = p + 2
    assert pack(ptrs, 124, 64, p, nb, None) == B


def test_nearest_index_rule_equals_interpolate():
    """(dst * in) / out in integers is what F.interpolate(mode="nearest") takes, for every in <= 1024 with out in {2 in - 1, 2 in}: the two sizes a stride-2 stage
    with padding can leave between neighbouring pyramid levels."""
    for n_in in range(1, 1025):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in {max(2 * n_in - 1, 1), 2 * n_in}:
            want = F.interpolate(src, size=(1, n_out), mode="nearest").view(-1).long().numpy()
            assert np.array_equal(br.nearest_index(n_out, n_in), want), (n_in, n_out)


# ------------------------------------------------------------------------------------------ the switch
def test_the_switch_is_off_by_default_and_adds_nothing_to_the_checkpoint():
    m = Backbone(list(bc.RETURN_LAYERS), use_fpn=True, fpn_dim=64)
    assert Backbone.hip_forward is False and m.hip_forward is False and "hip_forward" not in m.__dict__   # a class attribute until an instance sets it
    assert Backbone.hip_precision == "fp32" and Backbone.hip_output_layout == "channels_last"
    m.hip_forward = True
    assert Backbone.hip_forward is False and m.pack_count == 0 and len(m.state_dict()) == 124


def test_with_the_switch_set_cpu_tensors_and_grad_wanting_calls_stay_eager(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library path was taken")
    monkeypatch.setattr(_backbone_lib, "backbone_forward", no_library)
    monkeypatch.setattr(_backbone_lib, "pack_weights", no_library)
    imgs, _, _ = bc.build("sq32")
    x = torch.from_numpy(imgs)
    eager, hip = build_module("sq32"), build_module("sq32")
    hip.hip_forward = True
    with torch.no_grad():
        want, got = eager(x), hip(x)                      # a CPU tensor
        assert all(torch.equal(got[k], want[k]) for k in want) and hip._use_hip(x) is False
        hip64 = build_module("sq32", torch.float64)
        hip64.hip_forward = True
        assert hip64(x.double())["layer1"].dtype == torch.float64
    got = hip(x)                                          # gradients wanted: layer2 and the pyramid require them
    assert got["layer1"].requires_grad and not got["conv1"].requires_grad and torch.equal(got["layer2"].detach(), want["layer2"])
    (got["layer1"].sum() + got["layer2"].sum()).backward()
    assert hip.body["layer2"][0].conv1.weight.grad is not None and hip.fpn.inner_blocks[0][0].weight.grad is not None
    assert hip.body["layer1"][0].conv1.weight.grad is None and hip.pack_count == 0
