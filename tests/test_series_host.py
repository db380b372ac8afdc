"""Host side of the observable series: the numpy restatement in series_ref.py against a naive
implementation, and the estimators of flipcomplexityempirical_amd.diagnostics.  No GPU."""
import math

import numpy as np
import pytest

import series_ref
from flipcomplexityempirical_amd import diagnostics as dg

EPS = np.finfo(np.float64).eps
XMAX = 2_000_000  # the cut of a graph with two million edges


def naive(x, max_lag):
    """O(n * L) per series with Python integers; the terms from the same IEEE expression in
    Python floats, summed by math.fsum (exact), so only the order of the sum differs."""
    n, N = x.shape
    sums = np.zeros((N, 3, max_lag + 1), np.int64)
    t = [[0.0] * N for _ in range(max_lag + 3)]
    for j in range(N):
        col = [int(v) for v in x[:, j]]
        m = float(sum(col)) / float(n)
        for l in range(max_lag + 1):
            P = sum(col[s] * col[s + l] for s in range(n - l))
            A, B = sum(col[:n - l]), sum(col[l:])
            sums[j, :, l] = (P, A, B)
            t[l][j] = ((float(P) - m * float(A + B)) + float(n - l) * m * m) / float(n)
        t[max_lag + 1][j], t[max_lag + 2][j] = m, m * m
    pooled = np.array([math.fsum(row) for row in t])
    bound = np.array([(math.ceil(N / 256) + 8) * EPS * math.fsum(abs(v) for v in row)
                      for row in t])
    return sums, pooled, bound


def _random(N, n=24, hi=400, seed=0):
    return np.random.default_rng(seed + N).integers(0, hi, (n, N))


CASES = {
    "random_1": lambda: _random(1),
    "random_70": lambda: _random(70),
    "random_600": lambda: _random(600, n=12),
    "constant": lambda: np.full((24, 5), 137),
    "at_xmax": lambda: np.concatenate(
        [np.full((24, 1), XMAX),
         XMAX - np.random.default_rng(5).integers(0, 3, (24, 2))], axis=1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_series_ref_equals_naive(name):
    x = CASES[name]()
    n = x.shape[0]
    assert n * XMAX ** 2 < 2 ** 63
    max_lag = n - 1
    sums, pooled = series_ref.series_acf(x, max_lag)
    want_sums, want_pooled, bound = naive(x, max_lag)
    assert np.array_equal(sums, want_sums)
    err = np.abs(pooled[0] - want_pooled)
    print(name, "max err", err.max(), "max bound", bound.max())
    assert (err <= bound).all(), (err, bound)
    if name == "constant":
        assert not pooled[0, :max_lag + 1].any()  # c == 0 exactly
        assert pooled[0, max_lag + 1] == 137.0 * x.shape[1]


def test_by_rung_groups_and_regroup():
    """Group r of the by-rung pooling = the plain pooling of the slots set * R + r; regroup is
    the per-sample permutation."""
    R, S, n = 4, 3, 20
    rng = np.random.default_rng(3)
    x = rng.integers(0, 100, (n, R * S))
    # chain c is member c // S of set c % S; every set draws a permutation of the rungs per sample
    set_of = np.arange(R * S) % S
    rung = np.empty((n, R * S), np.int64)
    for t in range(n):
        for s in range(S):
            rung[t, s::S] = rng.permutation(R)
    y = series_ref.regroup(x, rung, set_of, R)
    for t in range(n):
        assert sorted(y[t].tolist()) == sorted(x[t].tolist())
        for c in range(R * S):
            assert y[t, set_of[c] * R + rung[t, c]] == x[t, c]
    sums, pooled = series_ref.series_acf(y, 5, n_rungs=R)
    assert pooled.shape == (R, 8)
    for r in range(R):
        want = series_ref.pooled(sums[r::R], n)[0]
        assert np.array_equal(pooled[r].view(np.uint64), want.view(np.uint64))


def _ar1_tau(seed, phi=0.8, M=64, n=4000, max_lag=200):
    rng = np.random.default_rng(seed)
    burn = 500
    e = rng.standard_normal((n + burn, M))
    y = np.zeros_like(e)
    for t in range(1, n + burn):
        y[t] = phi * y[t - 1] + e[t]
    x = np.rint(1000 + 50 * y[burn:]).astype(np.int64)
    assert x.min() >= 0
    _, pooled = series_ref.series_acf(x, max_lag)
    return dg.tau_int(dg.autocorrelation(pooled[0], M))


def test_tau_int_ar1():
    """64 AR(1) series (phi = 0.8, scaled by 50 and rounded to integers: the rounding noise is
    1/12 against a variance of 6,944), 4,000 samples, max_lag 200, numpy seed 7, against
    (1 + phi) / (1 - phi) = 9.

    The margin comes from the same estimator on 20 other seeds (100..119), run on the CPU when
    this test was written: mean 8.9021, standard deviation 0.1345, range [8.7557, 9.3199]
    (the mean sits 0.1 below 9: the means are removed per series, and Geyer's rule cuts the
    tail).  Margin = 4 standard deviations = 0.54; the value under test was not used."""
    phi, margin = 0.8, 4 * 0.1345
    tau = _ar1_tau(7)
    print("tau_int", tau)
    assert abs(tau - (1 + phi) / (1 - phi)) <= margin


def test_tau_int_truncation():
    assert dg.tau_int([1.0]) == 1.0
    assert dg.tau_int([1.0, 0.5, 0.25, 0.125]) == -1 + 2 * (1.5 + 0.375)
    # the pair (0.1, -0.2) is negative: it and everything after it is dropped
    assert dg.tau_int([1.0, 0.5, 0.1, -0.2, 0.9, 0.9]) == -1 + 2 * 1.5
    # an unpaired last lag is not used
    assert dg.tau_int([1.0, 0.5, 0.25]) == -1 + 2 * 1.5
    assert dg.ess(1000, 8, 4.0) == 2000.0


def test_round_trips_hand_written():
    R = 3
    paths = {
        # up and down twice
        (0, 1, 2, 1, 0, 1, 2, 2, 1, 0): 2,
        # starts at the top: counting begins at the first visit to rung 0; one full trip
        (2, 1, 0, 1, 2, 1, 0, 1): 1,
        # never reaches the top
        (0, 1, 0, 1, 1, 0): 0,
        # reaches the top, never returns
        (0, 1, 2, 2, 1, 1): 0,
        # never at the bottom
        (1, 2, 1, 2, 1, 2): 0,
    }
    n = max(len(p) for p in paths)
    cols = [list(p) + [p[-1]] * (n - len(p)) for p in paths]
    got = dg.round_trips(np.array(cols).T, R)
    assert got.tolist() == list(paths.values())
    # two rungs: every return to rung 0 after a visit to rung 1
    assert dg.round_trips(np.array([[0, 1, 0, 1, 0, 0, 1]]).T, 2).tolist() == [2]


def test_rhat_arithmetic():
    """rhat_from_sums on the pooled sums of series_ref against the textbook computation on
    the raw series; and the split form through a stand-in for a Chains handle."""
    rng = np.random.default_rng(11)
    n, M = 50, 6
    x = rng.integers(0, 200, (n, M)) + np.arange(M)[None, :] * 15  # means that differ

    def direct(x):
        n, M = x.shape
        xf = x.astype(np.float64)
        W = xf.var(axis=0, ddof=1).mean()
        B_over_n = xf.mean(axis=0).var(ddof=1)
        return math.sqrt(((n - 1) / n * W + B_over_n) / W)

    # two routes to the same variances: the pooled c[0] cancels P against n * m^2, a relative
    # error of about eps * mean^2 / variance ~ 1e-15 here; 1e-12 is rounding level, no more
    _, pooled = series_ref.series_acf(x, 0)
    got = dg.rhat_from_sums(pooled[0, 0], pooled[0, 1], pooled[0, 2], n, M)
    assert got == pytest.approx(direct(x), rel=1e-12)
    assert got > 1.05  # the shifted means show

    class Stub:  # what rhat() uses of a Chains handle
        n_chains, n_samples = M, n

        def series_acf(self, what, max_lag, by_rung=False, t0=0, n=None):
            return series_ref.series_acf(x[t0:t0 + n], max_lag)[1]

    h = n // 2
    halves = np.concatenate([x[:h], x[n - h:]], axis=1)
    assert dg.rhat(Stub(), "cut") == pytest.approx(direct(halves), rel=1e-12)
    assert dg.rhat(Stub(), "cut", split=False) == pytest.approx(direct(x), rel=1e-12)
