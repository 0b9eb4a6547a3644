"""What the drop-ins of the localisation head (matching.py, fine_matching.py, transformer.py) share: the cache of a module's packed weights, the precision and
device checks, and the matcher MLP (C -> 128 -> 128 -> 1) that the coarse and the fine matcher both pack into one image (nl_s2d_pack_weights)."""
from __future__ import annotations

import torch

from . import _lib

MATCHER_HIDDEN = 128
MATCHER_MLP_PARAMS = ("mlps.0.weight", "mlps.0.bias", "mlps.2.weight", "mlps.2.bias", "mlps.4.weight", "mlps.4.bias")


def check_precision(precision):
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}")
    return precision


def require_device(who, *tensors):
    """The eval path has no CPU form: refuse anything that is not on a HIP device."""
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who}'s eval path runs only on a HIP device (no CPU fallback); move the module and its inputs to cuda")


class PackedCache:
    """Mixin: a module's packed weights, keyed by device + (storage, version, dtype) of every parameter they were packed from."""

    def _cache_init(self):
        self._packed = None
        self._packed_key = None
        self.pack_count = 0   # how often the weights were packed (tests watch the cache)

    def _cached(self, device, params, pack):
        """params: the parameters in the order of the pack call; pack(ts) packs their fp32 device copies ts and returns the packed tensor."""
        key = (str(device),) + tuple((p.data_ptr(), p._version, p.dtype) for p in params)
        if self._packed is None or key != self._packed_key:
            ts = [p.detach().to(device=device, dtype=torch.float32).contiguous() for p in params]
            self._packed, self._packed_key = pack(ts), key
            self._pack_sources = ts   # alive until the stream has consumed them
            self.pack_count += 1
        return self._packed


def pack_matcher_mlp_train(who, module, device):
    """The training image of module.mlps (the transposed weights of nl_s2d_pack_train_weights, read by the backward calls of both matchers), cached in
    module._train_cache like the inference image."""
    def pack(ts):
        lib = _lib.load()
        need = lib.nl_s2d_train_weights_bytes(module.feat_dim)
        if need == 0:
            raise RuntimeError(f"{who}: feat_dim {module.feat_dim} is not supported by the HIP kernel (a multiple of 32, 32..256)")
        packed = torch.empty(need, dtype=torch.uint8, device=device)
        st = _lib.stream(device)
        _lib.check(lib.nl_s2d_pack_train_weights(module.feat_dim, ts[0].data_ptr(), ts[1].data_ptr(), packed.data_ptr(), need, st), "nl_s2d_pack_train_weights")
        return packed
    return module._train_cache._cached(device, [module.mlps[0].weight, module.mlps[2].weight], pack)


def matcher_mlp_grad_buffers(module, needs, device):
    """(the six parameters of module.mlps, an fp32 gradient buffer for each one whose entry of `needs` is set and None for the others: a NULL pointer in the
    backward call)."""
    params = [module.get_parameter(n) for n in MATCHER_MLP_PARAMS]
    return params, [torch.empty(p.shape, dtype=torch.float32, device=device) if need else None for p, need in zip(params, needs)]


def matcher_mlp_grads_out(params, grads):
    """The buffers of matcher_mlp_grad_buffers in their parameters' dtypes, as an autograd backward returns them."""
    return [None if g is None else g.to(p.dtype) for g, p in zip(grads, params)]


def new_train_cache():
    cache = PackedCache()
    cache._cache_init()
    return cache


def pack_matcher_mlp(who, module, device):
    """The packed image of module.mlps (a PackedCache module with feat_dim; who: its name in error messages), packed on the current stream when the cache misses."""
    def pack(ts):
        lib = _lib.load()
        need = lib.nl_s2d_packed_weights_bytes(module.feat_dim)
        if need == 0:
            raise RuntimeError(f"{who}: feat_dim {module.feat_dim} is not supported by the HIP kernel (a multiple of 32, 32..256)")
        packed = torch.empty(need, dtype=torch.uint8, device=device)
        st = _lib.stream(device)
        _lib.check(lib.nl_s2d_pack_weights(module.feat_dim, *[t.data_ptr() for t in ts], packed.data_ptr(), need, st), "nl_s2d_pack_weights")
        return packed
    return module._cached(device, [module.get_parameter(n) for n in MATCHER_MLP_PARAMS], pack)
