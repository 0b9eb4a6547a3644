"""Exact KNN with nodes pruned by the bounding box of their points (csrc/knn.hip, knn_nodes.h): idx and d2 bit for bit against
oracle/libknn_oracle.so on the smallest clouds that exercise each way a box of points differs from a cell — fewer points than K,
zero-volume and flat boxes, a dense fine cell beside single-point nodes, queries far outside the cloud, on a box face and on a
point, and the warm-start path along rays — and the records the build kernels leave in the frame memory against numpy."""
import numpy as np
import pytest
import torch

from tests.golden_cases import build_case
from tests.test_knn_node_records import CELLS, NODE_DTYPE, NODES, assert_nodes_equal, expected_nodes, surface_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    from nerf_loc_amd.renderer import HipRenderer
    case = build_case("tiny_full")
    cfg = case["cfg"]
    r = HipRenderer(cfg.W, cfg.C, cfg.S_total, "fp32")
    r.load_weights({k: torch.from_numpy(v) for k, v in case["weights"].items()})
    return r, case


def _set_support(renderer, p):
    r, case = renderer
    cfg, fr, m = case["cfg"], case["frame"], len(p)
    support = {"xyz": p, "feature": np.zeros((m, 195), np.float32), "confidence": np.ones((m, 1), np.float32), "direction": np.zeros((m, 4), np.float32)}
    r.set_frame(fr["topk_images"], fr["feat_fine_src"], fr["vis_featmaps"], fr["topk_Ks"], fr["topk_poses"], cfg.near, cfg.far, support)
    return r


def _check(renderer, p, q, K=8):
    from oracle import render_oracle as orc
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    r = _set_support(renderer, p)
    d2, idx = r.knn(q, K)
    d2o, idxo = orc.knn_points(torch.from_numpy(q), torch.from_numpy(p), K)
    assert np.array_equal(d2.cpu().numpy(), d2o.numpy())
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), idxo.numpy())
    return d2.cpu().numpy(), idx.cpu().numpy()


def _queries(rng, p, n=256):
    """around the cloud, far from it, and on the points themselves"""
    lo, hi = p.min(0), p.max(0)
    span = max(float((hi - lo).max()), 1e-3)
    q = rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (n, 3))
    q[::4] += rng.choice([-1.0, 1.0], (len(q[::4]), 3)) * 20 * span
    q[1::8] = p[rng.integers(0, len(p), len(q[1::8]))]
    return q.astype(np.float32)


@pytest.mark.parametrize("m", [3, 7])
def test_fewer_points_than_k(renderer, m):
    rng = np.random.default_rng(m)
    p = rng.standard_normal((m, 3)).astype(np.float32)
    d2, idx = _check(renderer, p, _queries(rng, p))
    assert not d2[:, m:].any() and not idx[:, m:].any(), "slots past the cloud stay (0, 0)"


def test_identical_points(renderer):
    rng = np.random.default_rng(9)
    p = np.repeat(rng.standard_normal((1, 3)), 9, 0).astype(np.float32)
    _check(renderer, p, _queries(rng, p))


def test_coplanar_points(renderer):
    rng = np.random.default_rng(64)
    p = np.concatenate([rng.uniform(-1, 1, (64, 2)), np.full((64, 1), 0.375)], 1).astype(np.float32)
    q = _queries(rng, p)
    q[2::8, 2] = 0.375   # in the plane
    _check(renderer, p, q)


def test_dense_cell_and_single_point_nodes(renderer):
    rng = np.random.default_rng(512)
    far = 10.0 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])
    p = np.concatenate([rng.uniform(-1e-3, 1e-3, (512, 3)), far]).astype(np.float32)
    q = np.concatenate([_queries(rng, p), rng.uniform(-2e-3, 2e-3, (128, 3)), far + rng.uniform(-0.5, 0.5, far.shape), 0.5 * far]).astype(np.float32)
    _check(renderer, p, q)


def test_sphere_shell(renderer):
    rng = np.random.default_rng(2000)
    p = rng.standard_normal((2000, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    u = rng.standard_normal((128, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = np.concatenate([np.zeros((4, 3)), rng.uniform(-1e-3, 1e-3, (60, 3)), u, p[:64], 10.0 * u]).astype(np.float32)
    _check(renderer, p, q)


def test_queries_on_box_faces_and_on_points(renderer):
    """A node's box faces lie at coordinates of its points: a query that takes each coordinate from some point is on a face of every
    node that point bounds (single-point nodes: on the box itself), inside or outside the box along the other two axes."""
    rng = np.random.default_rng(77)
    p = surface_cloud(1000, 77)
    i = rng.integers(0, len(p), (512, 3))
    q = np.stack([p[i[:, 0], 0], p[i[:, 1], 1], p[i[:, 2], 2]], 1)
    q[:128, 1:] = p[i[:128, 0], 1:] + rng.uniform(-0.3, 0.3, (128, 2)).astype(np.float32)   # one coordinate exact, near the point
    lo, hi = p.min(0), p.max(0)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    _check(renderer, p, np.concatenate([q, p[:256], corners]))


@pytest.mark.parametrize("K", [8, 1])
def test_rays_through_a_surface(renderer, K):
    """32 rays x 128 consecutive samples: every query after a wave's first takes its bound from its predecessor's neighbours"""
    rng = np.random.default_rng(5000)
    p = surface_cloud(5000, 5000)
    o = np.concatenate([rng.uniform(-1.5, 1.5, (32, 2)), np.full((32, 1), 3.0)], 1)
    d = np.concatenate([rng.uniform(-0.4, 0.4, (32, 2)), np.full((32, 1), -1.0)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.linspace(0.5, 6.0, 128)
    _check(renderer, p, (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3), K)


def test_built_records_match_numpy(renderer):
    """The grid lies in the frame memory behind the visibility maps (abi.hip: nl_frame_create; knn.hip: nl_knn_grid_build): parameters,
    starts, two scratch arrays, cell_of, the sorted points, the records — every block aligned to 256 bytes."""
    p = surface_cloud(1000, 1000)
    r = _set_support(renderer, p)
    torch.cuda.synchronize()
    visf, mem = r._frame_keep[2], r._frame_keep[4].cpu().numpy()
    al = lambda x: (x + 255) // 256 * 256
    off = al(visf.shape[0] * visf.shape[2] * visf.shape[3] * 32 * 4) + al(48)
    starts = mem[off: off + 4 * (CELLS + 1)].view(np.int32)
    off += al(4 * (CELLS + 1)) + 2 * al(4 * CELLS) + al(4 * len(p))
    sorted4 = mem[off: off + 16 * len(p)].view(np.float32).reshape(-1, 4)
    off += al(16 * len(p))
    nodes = mem[off: off + 32 * NODES].view(NODE_DTYPE)
    assert starts[0] == 0 and starts[-1] == len(p)
    assert np.array_equal(np.sort(sorted4[:, 3].copy().view(np.int32)), np.arange(len(p))), "the sorted array is a permutation of the cloud"
    assert_nodes_equal(nodes, expected_nodes(starts, sorted4))
