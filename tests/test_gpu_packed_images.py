"""GPU tests of the localisation head's packed weight images (nl_s2d_pack_weights, nl_fine_pack_proj, nl_sct_pack_weights through the modules' caches): every byte
of [0, layout.total) against an image built here, in numpy, from the documented layouts — s2d_layout (csrc/s2d.h), fine_proj_layout (csrc/fine.hip), sct_layout
(csrc/sct.hip), the two fragment maps (csrc/mfma.h) and s2d_unit — with round-to-nearest-even bf16 and fp16.  Nothing here calls the library for the expectation.

Shapes: the smallest at which an index mix-up still shows — the matcher MLP at C = 32 and 64 (one and two 32-wide k blocks of layer 1), the fine projection at
32 -> 64 and 64 -> 32 (nrb != 4, N != K), the transformer at d_model 64 / dim_feedforward 32 (in_proj 192 x 64, linear1 32 x 64, linear2 64 x 32)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 128   # hidden width of the matcher MLP
PLANTED = (1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, 2.0 ** -20, 1000.123)   # two bf16 ties (round to even: down, up), an fp16 subnormal, a large value


# ---------------------------------------------------------------------------------------------- number formats
def _bf16(v):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_planes(v):
    hi = _bf16(v)
    return hi, _bf16(v - (hi.astype(np.uint32) << 16).view(np.float32))   # lo = bf16(v - float(hi)), the subtraction in fp32


def _f16_planes(v):
    hi = v.astype(np.float16)
    return hi.view(np.uint16), (v - hi.astype(np.float32)).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------- fragment maps
def _unit(b, r, hh):
    """hidden unit held by accumulator register r of 32-block b in half-wave hh"""
    return 32 * b + 8 * (r >> 2) + 4 * hh + (r & 3)


def _frag16(w):
    """16-bit plane: fragment (s, rb), lane, slot j <-> W[32 rb + (lane & 31)][16 s + 8 (lane >> 5) + j]"""
    nrb = w.shape[0] // 32
    i = np.arange(w.size)
    j, lane, f = i & 7, (i >> 3) & 63, i >> 9
    return w[32 * (f % nrb) + (lane & 31), 16 * (f // nrb) + 8 * (lane >> 5) + j]


def _frag32(w):
    """fp32 plane: fragment (g, t, rb), lane <-> W[32 rb + (lane & 31)][8 g + 4 (lane >> 5) + t]"""
    nrb = w.shape[0] // 32
    i = np.arange(w.size)
    lane, f = i & 63, i >> 6
    return w[32 * (f % nrb) + (lane & 31), 8 * (f // (4 * nrb)) + 4 * (lane >> 5) + ((f // nrb) & 3)]


def _frag16_w2(w):
    """W2 (128 x 128), 16-bit: fragment (b, s, rb): slot j <-> the hidden unit of accumulator register 8 s + j of block b"""
    i = np.arange(w.size)
    j, lane, f = i & 7, (i >> 3) & 63, i >> 9
    return w[32 * (f & 3) + (lane & 31), _unit(f >> 3, 8 * ((f >> 2) & 1) + j, lane >> 5)]


def _frag32_w2(w):
    """W2, fp32: fragment (b, t, rb), lane <-> W2[32 rb + (lane & 31)][unit of accumulator register t of block b]"""
    i = np.arange(w.size)
    lane, f = i & 63, i >> 6
    return w[32 * (f & 3) + (lane & 31), _unit(f >> 6, (f >> 2) & 15, lane >> 5)]


class _Image:
    """Expected bytes [0, total) assembled from named pieces; every byte must be given exactly once."""

    def __init__(self, total):
        self.buf = np.zeros(total, np.uint8)
        self.given = np.zeros(total, bool)
        self.pieces = []

    def put(self, name, off, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert not self.given[off:off + raw.size].any(), name
        self.buf[off:off + raw.size] = raw
        self.given[off:off + raw.size] = True
        self.pieces.append((name, off, raw.size))
        return off + raw.size

    def check(self, tag, got):
        assert self.given.all(), f"{tag}: the expected image leaves bytes of [0, {self.buf.size}) open"
        assert got.size >= self.buf.size, f"{tag}: packed image has {got.size} bytes, the layout needs {self.buf.size}"
        for name, off, n in self.pieces:
            bad = np.nonzero(got[off:off + n] != self.buf[off:off + n])[0]
            assert bad.size == 0, f"{tag}: plane {name} differs in {bad.size} of {n} bytes, first at byte {int(bad[0])} of the plane"


# ---------------------------------------------------------------------------------------------- expected images
def _mlp_image(p, C):
    """s2d_layout(C): w1hi | w2hi | w2lo | small (2 KB) | w1lo | f32w1 | f32w2 | h1hi | h1lo | h2hi | h2lo"""
    w1, w2 = p["mlps.0.weight"], p["mlps.2.weight"]
    b1h, b1l = _bf16_planes(_frag16(w1))
    b2h, b2l = _bf16_planes(_frag16_w2(w2))
    h1h, h1l = _f16_planes(_frag16(w1))
    h2h, h2l = _f16_planes(_frag16_w2(w2))
    small = np.zeros(512, np.float32)   # b1p / b2p / w3p [hh][16 b + r] in accumulator order, then b3 and zero padding
    for which, src in enumerate((p["mlps.0.bias"], p["mlps.2.bias"], p["mlps.4.weight"].reshape(-1))):
        for hh in range(2):
            for b in range(4):
                for r in range(16):
                    small[128 * which + 64 * hh + 16 * b + r] = src[_unit(b, r, hh)]
    small[384] = p["mlps.4.bias"][0]
    img = _Image(2 * (4 * C * H + 4 * H * H) + 4 * (C * H + H * H) + 2048)
    o = 0
    for name, arr in (("w1hi", b1h), ("w2hi", b2h), ("w2lo", b2l), ("small", small), ("w1lo", b1l), ("f32w1", _frag32(w1)), ("f32w2", _frag32_w2(w2)),
                      ("h1hi", h1h), ("h1lo", h1l), ("h2hi", h2h), ("h2lo", h2l)):
        o = img.put(name, o, arr)
    assert o == img.buf.size
    return img


def _proj_image(w, b):
    """fine_proj_layout(Cf, Cout): bf16 hi | bf16 lo | fp32 | bias"""
    hi, lo = _bf16_planes(_frag16(w))
    img = _Image(8 * w.size + 4 * b.size)
    o = 0
    for name, arr in (("hi", hi), ("lo", lo), ("f32", _frag32(w)), ("bias", b)):
        o = img.put(name, o, arr)
    return img


def _sct_image(p, C, F):
    """sct_layout(C, F): per layer the four matrices (in_proj, out_proj, linear1, linear2), each fp16 hi | fp16 lo | bf16 | fp32, then the vectors: in_proj_bias,
    out_proj.bias, linear1.bias, linear2.bias and the weight / bias of the two LayerNorms the layer applies (decoder layers: norm2, norm3)."""
    layers = (("self_attn_layer0", "self_attn", "norm1", "norm2"), ("self_attn_layer1", "self_attn", "norm1", "norm2"),
              ("cross_attn_layer0", "multihead_attn", "norm2", "norm3"), ("cross_attn_layer1", "multihead_attn", "norm2", "norm3"))
    img = _Image(4 * (10 * (4 * C * C + 2 * C * F) + 4 * (9 * C + F)))
    o = 0
    for layer, attn, na, nb in layers:
        g = lambda n: p[f"{layer}.{n}"]
        for name in (f"{attn}.in_proj_weight", f"{attn}.out_proj.weight", "linear1.weight", "linear2.weight"):
            w = g(name)
            hi, lo = _f16_planes(_frag16(w))
            for plane, arr in (("f16 hi", hi), ("f16 lo", lo), ("bf16", _bf16(_frag16(w))), ("f32", _frag32(w))):
                o = img.put(f"{layer}.{name} {plane}", o, arr)
        for name in (f"{attn}.in_proj_bias", f"{attn}.out_proj.bias", "linear1.bias", "linear2.bias", f"{na}.weight", f"{na}.bias", f"{nb}.weight", f"{nb}.bias"):
            o = img.put(f"{layer}.{name}", o, g(name))
    assert o == img.buf.size
    return img


# ---------------------------------------------------------------------------------------------- weights
def _fill(module, seed):
    """Seeded normal values with the planted entries in every tensor that has room; returns {name: fp32 array}.  Parameters are pairwise distinct and so are the
    rows of every matrix, so a swapped tensor or row cannot pass."""
    rng = np.random.default_rng(seed)
    out = {}
    with torch.no_grad():
        for name, prm in module.named_parameters():
            v = rng.standard_normal(tuple(prm.shape)).astype(np.float32)
            flat = v.reshape(-1)
            if flat.size >= 8:
                for k, x in enumerate(PLANTED):
                    flat[(k * (flat.size // 4) + 3 * k + 1) % flat.size] = x * (-1.0 if k == 1 else 1.0)
            prm.copy_(torch.from_numpy(v))
            out[name] = v
    assert max(float(np.abs(v).max()) for v in out.values()) < 6e4   # no fp16 infinity
    vals = list(out.values())
    for a in range(len(vals)):
        if vals[a].ndim == 2:
            assert len({r.tobytes() for r in vals[a]}) == vals[a].shape[0]
        for b in range(a + 1, len(vals)):
            assert vals[a].shape != vals[b].shape or not np.array_equal(vals[a], vals[b])
    return out


def _packed(module, pack):
    module = module.to(DEV).eval()
    with torch.cuda.device(DEV):
        img = pack(module, torch.device(DEV))
        torch.cuda.synchronize()
    assert module.pack_count == 1 and module._packed is img
    return img.cpu().numpy()


@pytest.mark.parametrize("C", (32, 64))
def test_matcher_mlp_image_coarse(C):
    from nerf_loc_amd.matching import S2DMatching
    m = S2DMatching(C)
    p = _fill(m, 100 + C)
    _mlp_image(p, C).check(f"S2DMatching C={C}", _packed(m, lambda mod, dev: mod._packed_weights(dev)))


@pytest.mark.parametrize("C", (32, 64))
def test_matcher_mlp_image_fine(C):
    from nerf_loc_amd.fine_matching import FineMatching
    m = FineMatching({"correct_thr": 1.0, "loss_type": "l2", "feat_dim": C})
    p = _fill(m, 200 + C)
    _mlp_image(p, C).check(f"FineMatching C={C}", _packed(m, lambda mod, dev: mod._pack(dev)))


@pytest.mark.parametrize("Cf,Cout", ((32, 64), (64, 32)))
def test_fine_proj_image(Cf, Cout):
    from nerf_loc_amd.fine_matching import FinePreprocess
    m = FinePreprocess({"fine_concat_coarse_feat": False, "fine_window_size": 7, "in_channels_coarse": 64, "in_channels_fine": Cf, "out_channels": Cout})
    p = _fill(m, 300 + Cf)
    _proj_image(p["proj.weight"], p["proj.bias"]).check(f"FinePreprocess {Cf}->{Cout}", _packed(m, lambda mod, dev: mod._pack(dev)))


def test_transformer_image():
    from nerf_loc_amd.transformer import SelfCrossTransformer
    C, F = 64, 32
    m = SelfCrossTransformer(d_model=C, nhead=8, dim_feedforward=F, dropout=0.0)
    p = _fill(m, 400)
    assert len(p) == 52
    _sct_image(p, C, F).check("SelfCrossTransformer", _packed(m, lambda mod, dev: mod._pack(dev)))
