"""Compactness scores of sampled plans from their district geometry (host side, numpy float64).

GerryChain's ``GeographicPartition`` keeps ``cut_edges_by_part``, ``interior_boundaries``,
``exterior_boundaries``, ``perimeter``, ``area`` and ``polsby_popper`` per district, from the
``shared_perim`` edge attribute and the ``boundary_perim`` and ``area`` node attributes of a
census graph.  ``Chains.district_geometry()`` returns the exact integer form of these for every
chain, ``G [..., k, 5]`` with the field indices below; the functions here turn it into the usual
scores.  GerryChain is not a dependency, so these definitions are the contract:

* ``perimeters``      interior + exterior perimeter of a district
* ``polsby_popper``   4 pi A / P^2; NaN where P == 0
* ``cut_edge_share``  a district's cut edges over the plan's cut (half the sum over the
  districts, every cut edge lying on two of them), so the shares of a plan sum to 2

The device sums integers.  ``quantise`` turns measured lengths and areas into them: with
``w = quantise(lengths, s)`` the sums come back in units of 1 / s, and ``length_scale = s``
(``area_scale`` likewise) takes them back.  Every function works on the last axes, so one call
scores every chain.
"""
from __future__ import annotations

import numpy as np

# field indices of the last axis of ``Chains.district_geometry()``
NODES, CUT_EDGES, INTERIOR, EXTERIOR, AREA = range(5)
FIELDS = ("nodes", "cut_edges", "interior", "exterior", "area")
TOTAL_LIMIT = 2 ** 31  # an array's total must stay below it (32-bit district sums)


def quantise(values, scale=1) -> np.ndarray:
    """``round(values * scale)`` as int64.  ValueError for a negative or non-finite value, or a
    total of 2^31 or more (what ``Chains.set_geometry`` takes)."""
    v = np.asarray(values, np.float64)
    if not np.isfinite(v).all():
        raise ValueError("values must be finite")
    if not np.isfinite(scale) or scale <= 0:
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    if (v < 0).any():
        raise ValueError("values must be >= 0")
    q = np.rint(v * float(scale))
    if not np.isfinite(q).all() or float(q.sum()) >= TOTAL_LIMIT or (q >= TOTAL_LIMIT).any():
        raise ValueError("the quantised total must stay below 2^31: use a smaller scale")
    q = q.astype(np.int64)
    if int(q.sum()) >= TOTAL_LIMIT:
        raise ValueError("the quantised total must stay below 2^31: use a smaller scale")
    return q


def _geometry(G):
    g = np.asarray(G)
    if g.ndim < 2 or g.shape[-1] != 5:
        raise ValueError(f"district geometry must be [..., k, 5], got {g.shape}")
    return g.astype(np.float64)


def perimeters(G, length_scale=1) -> np.ndarray:
    """Interior + exterior perimeter per district, float64 [..., k], in the lengths' units."""
    g = _geometry(G)
    return (g[..., INTERIOR] + g[..., EXTERIOR]) / float(length_scale)


def polsby_popper(G, length_scale=1, area_scale=1) -> np.ndarray:
    """4 pi A / P^2 per district, float64 [..., k]; NaN where the perimeter is 0."""
    g = _geometry(G)
    p = perimeters(g, length_scale)
    a = g[..., AREA] / float(area_scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(p > 0, 4.0 * np.pi * a / np.where(p > 0, p * p, 1.0), np.nan)


def cut_edge_share(G) -> np.ndarray:
    """A district's cut edges over the plan's cut, float64 [..., k]; NaN for a plan without a
    cut edge."""
    g = _geometry(G)
    cut = g[..., CUT_EDGES]
    total = cut.sum(axis=-1, keepdims=True) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, cut / np.where(total > 0, total, 1.0), np.nan)


def district_cut_distribution(hist) -> np.ndarray:
    """``Chains.geometry_hist()`` rows [..., n_edges + 1] normalised to sum 1 (NaN rows where
    nothing was measured)."""
    h = np.asarray(hist, np.float64)
    tot = h.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tot > 0, h / np.where(tot > 0, tot, 1.0), np.nan)
