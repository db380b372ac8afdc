"""Host side of the pairwise plan distances (no GPU): the numpy reference the GPU tests compare
with, plancloud.py, and the five entry points' export, binding and refusals before the device."""
import re

import numpy as np
import pytest

import pairdist_ref
from flipcomplexityempirical_amd import _lib, plancloud

SYMBOLS = ("fw_chains_pairdist_async", "fw_chains_read_pairdist", "fw_chains_write_pairdist",
           "fw_chains_pairdist_reset", "fw_chains_pairdist_info")


def plans(seed=5, chains=7, n=45, k=3):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, k, (chains, n)).astype(np.int16)
    X[3] = X[1]  # two equal plans
    return X


def test_reference_equals_a_double_loop():
    X = plans()
    n = X.shape[1]
    a, b = [0, 1, 2, 3, 4, 5, 6], [6, 3, 3, 1]
    for bb in (None, b):
        D, rs, near, h = pairdist_ref.measure(X, n, a, bb)
        cols = a if bb is None else bb
        want = [[sum(int(X[i, v] != X[j, v]) for v in range(n)) for j in cols] for i in a]
        assert D.tolist() == want and D.dtype == np.int32
        assert rs.tolist() == [sum(r) for r in want] and rs.dtype == np.int64
        for i, row in enumerate(want):
            cand = [(d, j) for j, d in enumerate(row) if bb is not None or j != i]
            assert tuple(near[i]) == min(cand)
        counts = [0] * (n + 1)
        for i, row in enumerate(want):
            for j, d in enumerate(row):
                if bb is not None or j > i:
                    counts[d] += 1
        assert h.tolist() == counts and h.dtype == np.uint64
    # row blocks do not change the matrix
    assert np.array_equal(pairdist_ref.matrix(X, a, b, block=2), pairdist_ref.matrix(X, a, b))
    # a single member has no partner
    assert pairdist_ref.nearest(np.zeros((1, 1)), True).tolist() == [[-1, -1]]
    assert pairdist_ref.nearest(np.zeros((1, 1)), False).tolist() == [[0, 0]]


def test_distinct_plans_and_medoid():
    X = plans()
    D = pairdist_ref.matrix(X, np.arange(len(X)))
    cls, count = plancloud.distinct_plans(D)
    assert count == len(X) - 1
    assert cls.tolist() == [0, 1, 2, 1, 4, 5, 6]
    cls, count = plancloud.distinct_plans(np.zeros((4, 4), np.int32))
    assert cls.tolist() == [0, 0, 0, 0] and count == 1
    assert plancloud.medoid(pairdist_ref.rowsum(D)) == int(np.argmin(D.sum(axis=1)))
    assert plancloud.medoid([5, 2, 2, 9]) == 1
    with pytest.raises(ValueError):
        plancloud.distinct_plans(np.zeros((2, 3)))


def test_mean_pairwise():
    hist = np.zeros(11, np.uint64)
    hist[2], hist[4] = 3, 1
    assert plancloud.mean_pairwise(hist) == 2.5
    assert np.isnan(plancloud.mean_pairwise(np.zeros(5, np.uint64)))
    X = plans()
    D = pairdist_ref.matrix(X, np.arange(len(X)))
    h = pairdist_ref.hist(D, X.shape[1], True)
    assert plancloud.mean_pairwise(h) == pytest.approx(D[np.triu_indices(len(X), 1)].mean())


def test_classical_mds_recovers_three_points_on_a_line():
    x = np.array([0.0, 3.0, 7.0])
    D = np.abs(x[:, None] - x[None, :])
    Y, w = plancloud.classical_mds(D, 2)
    assert Y.shape == (3, 2) and w.shape == (2,)
    y = Y[:, 0]
    if y[0] > y[2]:
        y = -y  # up to sign
    assert np.allclose(y, x - x.mean(), atol=1e-9)
    assert np.allclose(Y[:, 1], 0.0, atol=1e-6) and abs(w[1]) < 1e-9
    assert w[0] == pytest.approx(((x - x.mean()) ** 2).sum())
    with pytest.raises(ValueError):
        plancloud.classical_mds(D, 4)


def test_energy_distance():
    X = plans()
    a = np.array([0, 1, 2, 4])
    Daa = pairdist_ref.matrix(X, a)
    assert plancloud.energy_distance(Daa, Daa, Daa) == 0.0
    # two far groups of near plans
    Y = np.zeros((6, 40), np.int16)
    Y[3:] = 1
    Y[1, 0], Y[4, 1] = 1, 0
    A, B = [0, 1, 2], [3, 4, 5]
    e = plancloud.energy_distance(pairdist_ref.matrix(Y, A, B), pairdist_ref.matrix(Y, A),
                                  pairdist_ref.matrix(Y, B))
    assert e > 70
    with pytest.raises(ValueError):
        plancloud.energy_distance(np.zeros((2, 2)), np.zeros((3, 3)), np.zeros((2, 2)))


def test_landmark_assign():
    D = np.array([[4, 2, 2], [0, 5, 1], [7, 7, 3]], np.int32)
    j, d = plancloud.landmark_assign(D)
    assert j.tolist() == [1, 0, 2] and d.tolist() == [2, 0, 3]


def test_pairdist_symbols_exported_and_reject_before_the_device():
    L = _lib.load()
    assert {name for name, _, _ in _lib.SIGNATURES} >= set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert re.search(r" pwd=[0-9a-f]{16}", _lib.build_info())
    buf = np.zeros(8, np.int64)
    ids = np.zeros(4, np.int32)
    assert L.fw_chains_pairdist_async(None, _lib.ptr(ids), 4, None, 0) == _lib.FW_EINVAL
    assert L.fw_chains_pairdist_async(None, None, 0, None, 0) == _lib.FW_EINVAL
    assert L.fw_chains_read_pairdist(None, _lib.PAIRDIST_MATRIX, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_write_pairdist(None, _lib.PAIRDIST_HIST, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_pairdist_reset(None) == _lib.FW_EINVAL
    assert L.fw_chains_pairdist_info(None, _lib.ptr(buf)) == _lib.FW_EINVAL
    assert L.fw_last_error().decode()
    assert (_lib.PAIRDIST_MATRIX, _lib.PAIRDIST_ROWSUM, _lib.PAIRDIST_NEAREST,
            _lib.PAIRDIST_HIST) == (0, 1, 2, 3)
