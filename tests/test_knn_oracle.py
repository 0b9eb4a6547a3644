"""KNN oracle (C restatement + numpy restatement) vs the reference's own knn_cpu.cpp (its outputs stored in tests/golden/knn_ref.npz) and brute force."""
import numpy as np
import pytest
import torch

from oracle import render_oracle as orc
from tests.golden_cases import KNN_CASES, knn_clouds, knn_key
from tests.util import load_golden


@pytest.mark.parametrize("n,m,K,dup", [(300, 500, 8, False), (200, 300, 8, True), (100, 5, 8, False), (64, 200, 1, False), (50, 40, 8, True)])
def test_c_oracle_equals_numpy_restatement(n, m, K, dup):
    q, p = knn_clouds(n + m, n, m, dup)
    d_np, i_np = orc.knn_points_np(q, p, K)
    lib = orc._load_knn_lib()
    assert lib, "oracle/libknn_oracle.so missing: run `make -C oracle`"
    d_c, i_c = orc.knn_points(torch.from_numpy(q), torch.from_numpy(p), K, threads=2)
    assert np.array_equal(d_np, d_c.numpy())
    assert np.array_equal(i_np, i_c.numpy())


@pytest.mark.parametrize("n,m,K,dup", KNN_CASES)
def test_c_oracle_equals_reference_knn_cpu(n, m, K, dup):
    q, p = knn_clouds(7 * n + m, n, m, dup)
    g = load_golden("knn_ref")
    d_r, i_r = g[knn_key(n, m, K, dup) + "_d2"], g[knn_key(n, m, K, dup) + "_idx"]
    d_c, i_c = orc.knn_points(torch.from_numpy(q), torch.from_numpy(p), K)
    assert np.array_equal(d_r, d_c.numpy()), "squared distances must be bit-exact incl. tie order"
    assert np.array_equal(i_r, i_c.numpy()), "the heap's (dist, idx) tuple order is reproduced exactly"
