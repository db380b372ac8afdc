"""Partisan scores of sampled plans from their district tallies (host side, numpy float64).

The reference imports ``Election``, ``mean_median`` and ``efficiency_gap`` from GerryChain and
gives every node two vote columns (grid_chain_sec11.py:223).  ``Chains.tallies()`` returns the
exact per-district sums of such columns for every chain; the functions here turn the sums of
two parties, A and B, into the usual scores.  GerryChain is not a dependency, so these
definitions are the contract.  With A, B the two parties' district sums of one plan:

* ``vote_shares``     A / (A + B); NaN where a district has no votes, and every score below
  propagates it
* ``seats``           #{districts with A > B} (a tie is nobody's seat)
* ``mean_median``     median(shares) - mean(shares)
* ``efficiency_gap``  with t = A + B per district: if A > B then wasted_A = A - t/2 and
  wasted_B = B, otherwise wasted_A = A and wasted_B = B - t/2; the gap is
  (sum wasted_B - sum wasted_A) / sum t

Every function takes arrays [..., k] and works on the last axis, so one call scores every
chain: ``mean_median(t[:, a], t[:, b])`` with ``t = chains.tallies()``.
"""
from __future__ import annotations

import numpy as np


def _pair(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or a.ndim < 1:
        raise ValueError(f"district sums must have equal shapes [..., k], got {a.shape} and {b.shape}")
    return a, b


def vote_shares(a, b) -> np.ndarray:
    """A / (A + B) per district; NaN where A + B == 0."""
    a, b = _pair(a, b)
    t = a + b
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(t > 0, a / np.where(t > 0, t, 1.0), np.nan)


def seats(a, b) -> np.ndarray:
    """Districts A wins outright, int64 [...]."""
    a, b = _pair(a, b)
    return (a > b).sum(axis=-1).astype(np.int64)


def mean_median(a, b) -> np.ndarray:
    """median(shares) - mean(shares), float64 [...]; NaN if any district has no votes."""
    s = vote_shares(a, b)
    bad = np.isnan(s)
    s0 = np.where(bad, 0.0, s)
    return np.where(bad.any(axis=-1), np.nan, np.median(s0, axis=-1) - s0.mean(axis=-1))


def efficiency_gap(a, b) -> np.ndarray:
    """(sum wasted_B - sum wasted_A) / sum (A + B), float64 [...]; NaN without any votes."""
    a, b = _pair(a, b)
    t = a + b
    a_wins = a > b
    wasted_a = np.where(a_wins, a - t / 2, a)
    wasted_b = np.where(a_wins, b, b - t / 2)
    total = t.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, (wasted_b.sum(axis=-1) - wasted_a.sum(axis=-1)) /
                        np.where(total > 0, total, 1.0), np.nan)


def seat_distribution(hist) -> np.ndarray:
    """``Chains.seat_hist()`` rows [..., k + 1] normalised to sum 1 (NaN rows where nothing was
    tallied)."""
    h = np.asarray(hist, np.float64)
    tot = h.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tot > 0, h / np.where(tot > 0, tot, 1.0), np.nan)
