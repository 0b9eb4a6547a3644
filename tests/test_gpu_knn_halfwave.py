"""Exact KNN (csrc/knn.hip), idx and d2 bit for bit against oracle/libknn_oracle.so through the ordinary search entry, on the cases
written for a search that answers two queries per wave, one per 32-lane half (built, measured and not kept: DESIGN 5.1) — the
smallest inputs at which queries that share a wave can go wrong: fewer points than K and a wave with fewer queries than it has room
for, chains of consecutive queries that end in the middle of a wave, exact ties in a dense fine cell (more candidates within the
bound than a 32-entry deferred list holds), neighbouring queries whose searches differ as much as possible, a frontier that
overflows into coarse leaves, and the same queries in one call and in two (no result may depend on where in a wave or a chain a
query lands).  The one-query-per-wave kernel passes them, and whatever replaces it has to.  The clouds and queries are plain
functions: the oracle is checked on each of them against a brute-force fp32 restatement in test_oracle_handles_the_clouds, on the
CPU."""
import numpy as np
import pytest
import torch

from tests.golden_cases import build_case
from tests.test_knn_node_records import surface_cloud


def tiny_clouds():
    """M = 1, 7 (< K), 8 with N = 5: empty slots, and with four queries per half a second half that holds one query or none"""
    out = []
    for m in (1, 7, 8):
        rng = np.random.default_rng(100 + m)
        out.append((f"m{m}", rng.standard_normal((m, 3)).astype(np.float32), rng.uniform(-2, 2, (5, 3)).astype(np.float32)))
    return out


def ragged_counts():
    """N below one half's chain, N that leaves half 1 empty / partly filled, N that is no multiple of a wave's queries"""
    rng = np.random.default_rng(31)
    p = surface_cloud(600, 31)
    lo, hi = p.min(0), p.max(0)
    return [(f"n{n}", p, rng.uniform(lo - 0.3, hi + 0.3, (n, 3)).astype(np.float32)) for n in (1, 3, 4, 5, 13, 37, 263)]


def tie_cloud():
    """64 identical points and 8 others: exact ties; the 64 share one fine cell, which is scanned as a range with more than 32 candidates
    of one half within the bound (the deferred list pours)"""
    rng = np.random.default_rng(64)
    c = np.array([[0.25, -0.5, 0.125]])
    p = np.concatenate([np.repeat(c, 64, 0), c + rng.uniform(0.5, 1.0, (8, 3)) * rng.choice([-1.0, 1.0], (8, 3))]).astype(np.float32)
    step = np.linspace(0.0, 0.4, 16)[:, None] * np.array([[1.0, 0.5, -0.25]])
    q = np.concatenate([c + step, c - step, p[60:], c + rng.uniform(-3, 3, (24, 3))]).astype(np.float32)   # chains walking away from the tie
    return "ties", rng.permutation(p), q


def unequal_pair():
    """one half inside a dense cluster, the other far outside the bounding box: the most unequal trip counts of two halves, both ways round"""
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.uniform(-0.02, 0.02, (1500, 3)), rng.uniform(-1, 1, (500, 3))]).astype(np.float32)
    inside = rng.uniform(-0.02, 0.02, (4, 3))
    far = np.array([[40.0, -35.0, 50.0]]) + rng.uniform(-1, 1, (4, 3))
    q = np.concatenate([inside, far, far, inside, np.stack([inside, far], 1).reshape(-1, 3)]).astype(np.float32)
    return "unequal", p, q


def clustered_cloud():
    """4096 points in six fine cells, queries in the empty space between and around them"""
    rng = np.random.default_rng(4096)
    centres = rng.uniform(-1, 1, (6, 3))
    p = (centres[rng.integers(0, 6, 4096)] + rng.uniform(-2e-3, 2e-3, (4096, 3))).astype(np.float32)
    q = np.concatenate([rng.uniform(-1.2, 1.2, (96, 3)), centres.mean(0, keepdims=True), 0.5 * (centres[:3] + centres[3:])]).astype(np.float32)
    return "clustered", p, q


def shell_cloud():
    """4096 points on a sphere, queries at and near its centre: every node the shell crosses lies within the bound, a level's frontier passes
    what a half holds (64 nodes) and the rest is scanned as coarse leaves"""
    rng = np.random.default_rng(40)
    p = rng.standard_normal((4096, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    q = np.concatenate([np.zeros((2, 3)), rng.uniform(-1e-3, 1e-3, (6, 3)), p[:4] * 0.5, np.zeros((1, 3))]).astype(np.float32)
    return "shell", p, q


def all_cases():
    return tiny_clouds() + ragged_counts() + [tie_cloud(), unequal_pair(), clustered_cloud(), shell_cloud()]


def brute_force(p, q, K=8):
    """the definition at the top of knn.hip: the K smallest (dist2 bits, idx), dist2 = ((dx*dx) + dy*dy) + dz*dz in fp32, slots past M zero"""
    d = q[:, None, :].astype(np.float32) - p[None, :, :].astype(np.float32)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]
    d2o, idxo = np.zeros((len(q), K), np.float32), np.zeros((len(q), K), np.int64)
    for n in range(len(q)):
        order = np.lexsort((np.arange(len(p)), d2[n]))[:K]
        d2o[n, :len(order)], idxo[n, :len(order)] = d2[n, order], order
    return d2o, idxo


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c[0])
def test_oracle_handles_the_clouds(case):
    from oracle import render_oracle as orc
    _, p, q = case
    d2o, idxo = orc.knn_points(torch.from_numpy(q), torch.from_numpy(p), 8)
    d2b, idxb = brute_force(p, q)
    assert np.array_equal(d2o.numpy(), d2b) and np.array_equal(idxo.numpy(), idxb)


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


@pytest.mark.gpu
@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c[0])
def test_bit_exact_against_the_oracle(renderer, case):
    from oracle import render_oracle as orc
    _, p, q = case
    r = _set_support(renderer, p)
    d2, idx = r.knn(q, 8)
    d2o, idxo = orc.knn_points(torch.from_numpy(q), torch.from_numpy(p), 8)
    assert np.array_equal(d2.cpu().numpy(), d2o.numpy())
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), idxo.numpy())
    if len(p) < 8:
        assert not d2.cpu().numpy()[:, len(p):].any() and not idx.cpu().numpy()[:, len(p):].any(), "slots past the cloud stay (0, 0)"


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 5, 131])
def test_one_call_equals_two_calls(renderer, split):
    """rays through a surface: the chains are warm-started, and a split at an odd index moves every later query to another half, chain position and wave"""
    rng = np.random.default_rng(262)
    p = surface_cloud(3000, 262)
    o = np.concatenate([rng.uniform(-1.5, 1.5, (4, 2)), np.full((4, 1), 3.0)], 1)
    d = np.concatenate([rng.uniform(-0.4, 0.4, (4, 2)), np.full((4, 1), -1.0)], 1)
    q = (o[:, None, :] + d[:, None, :] * np.linspace(0.5, 6.0, 66)[None, :, None]).reshape(-1, 3).astype(np.float32)[:263]
    r = _set_support(renderer, p)
    d2, idx = (t.cpu().numpy() for t in r.knn(q, 8))
    parts = [[t.cpu().numpy() for t in r.knn(np.ascontiguousarray(part), 8)] for part in (q[:split], q[split:])]
    assert np.array_equal(d2, np.concatenate([parts[0][0], parts[1][0]])) and np.array_equal(idx, np.concatenate([parts[0][1], parts[1][1]]))
