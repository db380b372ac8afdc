"""Distances between plans from their overlap matrices (host side, numpy float64).

``Chains.overlap_matrix()`` returns, for every chain, the exact integer table
O[d, e] = #{nodes the reference labels d and the current plan labels e}; its row sums are the
reference's district sizes, its column sums the current ones, its total n.  Everything here
takes such a table, [k, k] or with leading axes [..., k, k], and works along the last two.

The reference's paper asks how long a flip chain takes to forget its plan: ``hamming`` and
``retention`` against a snapshot fall from 0 / 1 towards the level two independent chains
show (``Chains.overlap("partner")``), whatever the cut count's autocorrelation says.
"""
from __future__ import annotations

import numpy as np


def _table(O) -> np.ndarray:
    O = np.asarray(O, np.float64)
    if O.ndim < 2 or O.shape[-1] != O.shape[-2]:
        raise ValueError(f"an overlap table is [..., k, k], got {O.shape}")
    return O


def hamming(O) -> np.ndarray:
    """Nodes the two plans label differently: n - trace(O)."""
    O = _table(O)
    return O.sum(axis=(-2, -1)) - np.trace(O, axis1=-2, axis2=-1)


def retention(O) -> np.ndarray:
    """[..., k]: the share of reference district d that is still labelled d, O[d, d] / row sum
    (nan for an empty reference district)."""
    O = _table(O)
    rows = O.sum(axis=-1)
    diag = np.diagonal(O, axis1=-2, axis2=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rows > 0, diag / rows, np.nan)


def matched_distance(O) -> np.ndarray:
    """n minus the largest matched diagonal over all relabellings of the current plan's
    districts: the Hamming distance that does not care which district carries which name
    (an assignment problem; ``scipy.optimize.linear_sum_assignment``)."""
    from scipy.optimize import linear_sum_assignment  # lazy: delaunay_graph needs scipy too
    O = _table(O)
    flat = O.reshape((-1,) + O.shape[-2:])
    out = np.empty(len(flat), np.float64)
    for i, t in enumerate(flat):
        r, c = linear_sum_assignment(t, maximize=True)
        out[i] = t.sum() - t[r, c].sum()
    return out.reshape(O.shape[:-2])


def variation_of_information(O) -> np.ndarray:
    """H(R | X) + H(X | R) = 2 H(R, X) - H(R) - H(X) in nats, of the two labellings of the n
    nodes: 0 iff the plans are equal up to district names."""
    O = _table(O)
    n = O.sum(axis=(-2, -1), keepdims=True)

    def entropy(p, axes):
        with np.errstate(divide="ignore", invalid="ignore"):
            return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=axes)

    p = O / n
    vi = 2 * entropy(p, (-2, -1)) - entropy(p.sum(axis=-1), -1) - entropy(p.sum(axis=-2), -1)
    return np.maximum(vi, 0.0)


def distance_distribution(hist) -> dict:
    """Of a distance histogram ``Chains.distance_hist()`` [n_groups, n + 1] (or one row):
    per group the number of measured plans, the mean and the standard deviation of the
    distance, and its probability mass function."""
    h = np.atleast_2d(np.asarray(hist, np.float64))
    total = h.sum(axis=1)
    d = np.arange(h.shape[1], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pmf = np.where(total[:, None] > 0, h / total[:, None], np.nan)
    mean = (pmf * d).sum(axis=1)
    var = (pmf * (d - mean[:, None]) ** 2).sum(axis=1)
    return {"count": total, "mean": mean, "std": np.sqrt(var), "pmf": pmf}
