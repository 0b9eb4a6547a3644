"""The per-node records of the exact KNN's octree (nerf_loc_amd/csrc/knn_nodes.h) against numpy, on the CPU.

The record arithmetic lives in host-and-device functions; the build kernels of knn.hip only map threads to nodes.  This test compiles the
header alone with the host compiler, walks the nodes bottom-up the way the kernels do and compares every record of a 1 000-point cloud
with a direct restatement: a node's start and count are its `starts[]` range, its box is the min / max of exactly those points.
(tests/test_gpu_knn_node_bounds.py checks the records the kernels themselves leave in the frame memory against the same restatement.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf_loc_amd", "csrc")
DEPTH = 6
CELLS = 1 << (3 * DEPTH)
NODES = (8 ** (DEPTH + 1) - 1) // 7
NODE_DTYPE = np.dtype([("start", "<i4"), ("count", "<i4"), ("mn", "<f4", 3), ("mx", "<f4", 3)])

SHIM = r"""
#include "knn_nodes.h"
static_assert(sizeof(NlKnnNode) == 32, "two 16-byte halves");
extern "C" int shim_nodes() { return NL_KNN_NODES; }
extern "C" void shim_build(const int* starts, const float* sorted4, NlKnnNode* nodes) {
  for (int cell = 0; cell < (1 << (3 * NL_KNN_DEPTH)); ++cell) nl_knn_node_from_points(nodes, starts, sorted4, cell);
  for (int d = NL_KNN_DEPTH - 1; d >= 0; --d)
    for (int m = 0; m < (1 << (3 * d)); ++m) nl_knn_node_from_children(nodes, nl_knn_node_base(d) + m);
}
"""


def node_base(d):
    return (8 ** d - 1) // 7


def morton_sort(p):
    """starts (CELLS + 1,) and the sorted points (M, 4: x, y, z, index bits) of a 64^3 grid over the cloud's bounding box."""
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    cell = (ext / 64 if ext > 0 else 1.0) * 1.0001
    c = np.clip(np.floor((p - lo) / cell).astype(np.int64), 0, 63)
    code = np.zeros(len(p), np.int64)
    for b in range(DEPTH):
        for a in range(3):
            code |= ((c[:, a] >> b) & 1) << (3 * b + a)
    order = np.argsort(code, kind="stable")
    starts = np.zeros(CELLS + 1, np.int32)
    starts[1:] = np.cumsum(np.bincount(code, minlength=CELLS))
    sorted4 = np.empty((len(p), 4), np.float32)
    sorted4[:, :3] = p[order]
    sorted4[:, 3] = order.astype(np.int32).view(np.float32)
    return starts, sorted4


def expected_nodes(starts, sorted4):
    """Every record from its definition: depth d, Morton prefix m -> the range starts[m << 3 (6 - d)] .. starts[(m + 1) << 3 (6 - d)]."""
    out = np.zeros(NODES, NODE_DTYPE)
    out["mn"], out["mx"] = np.float32(3.4e38), np.float32(-3.4e38)
    for d in range(DEPTH + 1):
        edges = starts[:: 8 ** (DEPTH - d)]
        s, n = edges[:-1], np.diff(edges)
        rec = out[node_base(d): node_base(d + 1)]
        rec["start"], rec["count"] = s, n
        for m in np.nonzero(n)[0]:
            pts = sorted4[s[m]: s[m] + n[m], :3]
            rec["mn"][m], rec["mx"][m] = pts.min(0), pts.max(0)
    return out


def assert_nodes_equal(got, want):
    assert np.array_equal(got["start"], want["start"])
    assert np.array_equal(got["count"], want["count"])
    assert int(want["count"][0]) == int(want["count"][node_base(DEPTH):].sum()), "the root holds every point"
    full = want["count"] > 0
    assert np.array_equal(got["mn"][full], want["mn"][full]) and np.array_equal(got["mx"][full], want["mx"][full])
    # empty nodes: the identity of the min / max reduction (the search rejects them by their count)
    assert np.all(got["mn"][~full] == np.float32(3.4e38)) and np.all(got["mx"][~full] == np.float32(-3.4e38))


def surface_cloud(m, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2, 2, (m, 2))
    return np.concatenate([xy, 0.2 * np.sin(2 * xy[:, :1]) * np.cos(2 * xy[:, 1:])], 1).astype(np.float32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("knn_nodes")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "libshim.so"
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, str(d / "shim.cpp"), "-o", str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lib = ctypes.CDLL(str(so))
    assert lib.shim_nodes() == NODES
    return lib


@pytest.mark.parametrize("kind", ["surface", "identical", "dense_cell"])
def test_node_records_match_numpy(shim, kind):
    p = surface_cloud(1000, 3)
    if kind == "identical":
        p = np.repeat(p[:1], 9, 0)
    if kind == "dense_cell":   # 512 points in one fine cell and 8 single-point nodes far away
        rng = np.random.default_rng(4)
        p = np.concatenate([rng.uniform(-1e-3, 1e-3, (512, 3)), 10.0 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])]).astype(np.float32)
    starts, sorted4 = morton_sort(p)
    assert starts[-1] == len(p)
    got = np.zeros(NODES, NODE_DTYPE)
    shim.shim_build(starts.ctypes.data_as(ctypes.c_void_p), sorted4.ctypes.data_as(ctypes.c_void_p), got.ctypes.data_as(ctypes.c_void_p))
    assert_nodes_equal(got, expected_nodes(starts, sorted4))
