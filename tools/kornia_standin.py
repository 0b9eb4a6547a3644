"""A stand-in for the two kornia functions the reference's fine_matching.py imports, for machines without kornia (tools/gen_fine_golden.py).

Written from kornia's documented behaviour, not from its source:
  kornia.utils.grid.create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=None) -> (1, H, W, 2): the pixel coordinate grid, x in channel 0,
      y in channel 1, both in [-1, 1] when normalized_coordinates is set, else in pixels.
  kornia.geometry.subpix.dsnt.spatial_expectation2d(input (B, N, H, W), normalized_coordinates=True) -> (B, N, 2): the expected (x, y) of each heat-map, i.e. the
      sum over pixels of the coordinate grid times the (already normalised) heat-map.
install() registers modules under those names in sys.modules.
"""
import sys
import types

import torch


def create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=None):
    if normalized_coordinates:
        xs = torch.linspace(-1, 1, width, device=device, dtype=dtype)
        ys = torch.linspace(-1, 1, height, device=device, dtype=dtype)
    else:
        xs = torch.linspace(0, width - 1, width, device=device, dtype=dtype)
        ys = torch.linspace(0, height - 1, height, device=device, dtype=dtype)
    return torch.stack([xs[None, :].expand(height, width), ys[:, None].expand(height, width)], dim=-1).unsqueeze(0)


def spatial_expectation2d(input, normalized_coordinates=True):
    b, n, h, w = input.shape
    grid = create_meshgrid(h, w, normalized_coordinates, input.device, input.dtype).reshape(1, 1, h * w, 2)
    flat = input.reshape(b, n, h * w, 1)
    return (grid * flat).sum(dim=2)


def install():
    mods = {}
    for name in ("kornia", "kornia.geometry", "kornia.geometry.subpix", "kornia.geometry.subpix.dsnt", "kornia.utils", "kornia.utils.grid"):
        mods[name] = types.ModuleType(name)
    mods["kornia"].geometry, mods["kornia"].utils = mods["kornia.geometry"], mods["kornia.utils"]
    mods["kornia.geometry"].subpix = mods["kornia.geometry.subpix"]
    mods["kornia.geometry.subpix"].dsnt = mods["kornia.geometry.subpix.dsnt"]
    mods["kornia.utils"].grid = mods["kornia.utils.grid"]
    mods["kornia.geometry.subpix.dsnt"].spatial_expectation2d = spatial_expectation2d
    mods["kornia.utils.grid"].create_meshgrid = create_meshgrid
    sys.modules.update(mods)
