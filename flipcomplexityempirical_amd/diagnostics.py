"""Convergence diagnostics from the pooled output of ``Chains.series_acf``.

Pure numpy on a handful of doubles: the device has already reduced the series (the exact
lagged sums and their pooled autocovariances, include/flipwalk.h); what is left is the
arithmetic of the estimators.

A pooled row is ``[sum_j c_j[0..max_lag], sum_j m_j, sum_j m_j**2]`` over the ``n_series``
members of a group, with c_j[l] the lag-l autocovariance of series j about its own mean
(divided by n, the biased form) and m_j its mean over the n samples of the window.
"""
from __future__ import annotations

import numpy as np


def autocorrelation(pooled, n_series: int) -> np.ndarray:
    """rho(l) = sum c[l] / sum c[0], l = 0..max_lag, of one pooled row or of every row of a
    [n_groups, max_lag + 3] array.  The pooled sums of numerator and denominator run over
    the same ``n_series`` series, so the count cancels; it is checked, not used.  A group
    whose series are all constant (sum c[0] == 0) has no autocorrelation: NaN."""
    if int(n_series) < 1:
        raise ValueError("n_series must be >= 1")
    p = np.asarray(pooled, np.float64)
    c = p[..., :-2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / c[..., :1]


def tau_int(rho) -> float:
    """Integrated autocorrelation time 1 + 2 * sum_{l >= 1} rho(l) of one rho(0..L),
    truncated by Geyer's initial positive sequence: the pairs G_k = rho(2k) + rho(2k+1) are
    summed while they are positive (tau = -1 + 2 * sum G_k).  An unpaired last lag is not
    used."""
    r = np.asarray(rho, np.float64)
    if r.ndim != 1 or r.size < 1:
        raise ValueError("tau_int takes one autocorrelation function rho[0..L]")
    total = 0.0
    for k in range(r.size // 2):
        g = float(r[2 * k] + r[2 * k + 1])
        if not g > 0.0:
            break
        total += g
    if r.size < 2:  # lag 0 alone: no pair to sum
        return 1.0
    return -1.0 + 2.0 * total


def ess(n: int, n_series: int, tau: float) -> float:
    """Effective sample size of n samples of each of n_series independent series."""
    return float(n) * float(n_series) / float(tau)


def rhat_from_sums(sum_c0: float, sum_m: float, sum_m2: float, n: int, n_series: int) -> float:
    """Gelman-Rubin R-hat of ``n_series`` series of ``n`` samples from the pooled sums:
    W = n / (n - 1) * sum c[0] / M (the mean unbiased within-series variance), B / n = the
    unbiased variance of the M means, R-hat = sqrt(((n - 1) / n * W + B / n) / W)."""
    M, n = int(n_series), int(n)
    if M < 2 or n < 2:
        raise ValueError("R-hat needs at least 2 series of at least 2 samples")
    W = float(n) / (n - 1) * float(sum_c0) / M
    b_over_n = (float(sum_m2) - float(sum_m) * float(sum_m) / M) / (M - 1)
    return float(np.sqrt(((n - 1) / float(n) * W + b_over_n) / W))


def rhat(ch, what, by_rung: bool = False, split: bool = True, t0: int = 0, n=None):
    """R-hat of the recorded series of a ``Chains`` handle over the window (default: all
    samples): a float, or with ``by_rung`` one per rung.  ``split`` (the default) halves the
    window, floor(n / 2) samples at either end, and treats the halves of every series as
    series of their own: two ``max_lag = 0`` reductions on the device."""
    t0 = int(t0)
    n = ch.n_samples - t0 if n is None else int(n)
    if split:
        h = n // 2
        rows = ch.series_acf(what, 0, by_rung=by_rung, t0=t0, n=h) + \
            ch.series_acf(what, 0, by_rung=by_rung, t0=t0 + n - h, n=h)
        n_eff, mult = h, 2
    else:
        rows = ch.series_acf(what, 0, by_rung=by_rung, t0=t0, n=n)
        n_eff, mult = n, 1
    members = ch.n_chains // rows.shape[0] * mult
    out = np.array([rhat_from_sums(r[0], r[1], r[2], n_eff, members) for r in rows])
    return out if by_rung else float(out[0])


def round_trips(rung_series, n_rungs: int) -> np.ndarray:
    """Per chain (column of int [n, n_chains] rung samples), the completed excursions
    bottom rung -> top rung -> bottom rung.  A chain counts from its first visit to rung 0."""
    r = np.asarray(rung_series)
    if r.ndim != 2:
        raise ValueError("rung_series must be [n, n_chains]")
    top = int(n_rungs) - 1
    count = np.zeros(r.shape[1], np.int64)
    # 0: not yet at the bottom, 1: left the bottom, top not reached, 2: top reached
    state = np.zeros(r.shape[1], np.int8)
    for row in r:
        bottom, at_top = row == 0, row == top
        count += (state == 2) & bottom
        state = np.where(bottom, 1, np.where(at_top & (state == 1), 2, state)).astype(np.int8)
    return count
