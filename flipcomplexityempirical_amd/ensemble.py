"""Maps across the ensemble from the census arrays of ``Chains`` (``node_occupancy``,
``edge_cut_counts``, ``boundary_counts``, ``census_counts``).  Pure numpy: the device only counts.

Every function takes the arrays as read, with the leading group axis ([n_groups, ...]: one
group, or one per rung under a ladder), or one group's slice; ``cnt`` broadcasts against it.
A group nothing was counted in gives NaN frequencies.
"""
from __future__ import annotations

import numpy as np


def _ratio(counts, cnt, extra_axes):
    c = np.asarray(cnt, np.float64).reshape(np.shape(cnt) + (1,) * extra_axes)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(counts, np.float64) / c


def occupancy_frequency(occ, cnt) -> np.ndarray:
    """occ / cnt: the fraction of the counted plans that put node v in district d
    ([.., n, k]; each node's row sums to 1)."""
    return _ratio(occ, cnt, 2)


def part_sum_map(occ, label_values=None) -> np.ndarray:
    """The ensemble ``part_sum`` map sum_d value_d occ[.., v, d] as int64 [.., n]: the
    reference's per-node sum of assignment values (grid_chain_sec11.py:396-400), taken over the
    counted plans instead of over one chain's steps.  ``label_values``: the assignment value of
    each district index, as for ``Chains.enable_maps`` (default 0..k-1; {-1, 1} for the
    reference's k = 2 plans)."""
    occ = np.asarray(occ)
    k = occ.shape[-1]
    lv = np.arange(k, dtype=np.int64) if label_values is None else np.asarray(label_values, np.int64)
    if lv.shape != (k,):
        raise ValueError(f"need {k} label values")
    return occ.astype(np.int64) @ lv


def occupancy_entropy(occ, cnt) -> np.ndarray:
    """Per-node entropy -sum_d f log f (nats) of the occupancy frequencies, [.., n]: 0 where a
    node never changes district, log k where it is in each equally often."""
    f = occupancy_frequency(occ, cnt)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(f > 0, f * np.log(f), 0.0)
    return np.where(np.isnan(f).any(axis=-1), np.nan, -t.sum(axis=-1))


def edge_cut_frequency(ecut, cnt) -> np.ndarray:
    """ecut / cnt: the fraction of the counted plans that cut edge e ([.., n_edges]; the
    ensemble counterpart of the reference's cut_times plot)."""
    return _ratio(ecut, cnt, 1)


def boundary_frequency(bnd, cnt) -> np.ndarray:
    """bnd / cnt: the fraction of the counted plans with node v on a district boundary."""
    return _ratio(bnd, cnt, 1)


def symmetry_deviation(occ, cnt, perms, label_perms=None) -> float:
    """The largest |f - mean over perms of f o perm| of the occupancy frequencies: 0 when the
    occupancy is invariant under every node permutation of ``perms`` (int [m, n]; include the
    identity for the group average).  On a grid with a symmetric seed the stationary occupancy
    is invariant under the grid's symmetries, so this measures how far the ensemble is from it.
    ``label_perms`` int [m, k]: the district relabelling that goes with each node permutation
    (default: none), f o perm = f[.., perm, :][.., label_perm]."""
    f = occupancy_frequency(occ, cnt)
    perms = np.asarray(perms, np.int64)
    k = f.shape[-1]
    lp = (np.tile(np.arange(k), (len(perms), 1)) if label_perms is None
          else np.asarray(label_perms, np.int64))
    mean = sum(f[..., p, :][..., q] for p, q in zip(perms, lp)) / len(perms)
    return float(np.nanmax(np.abs(f - mean)))


def grid_symmetries(h: int, w: int) -> np.ndarray:
    """The node permutations of the h x w grid graph's symmetries (row-major node ids): the
    four of a rectangle, the eight of a square; the identity first."""
    idx = np.arange(h * w).reshape(h, w)
    out = [idx, idx[::-1], idx[:, ::-1], idx[::-1, ::-1]]
    if h == w:
        out += [m.T for m in list(out)]
    return np.stack([m.ravel() for m in out])


def node_image(values, h: int, w: int) -> np.ndarray:
    """A node map [.., h w] of the h x w grid graph as images [.., h, w]."""
    v = np.asarray(values)
    if v.shape[-1] != h * w:
        raise ValueError(f"{v.shape[-1]} nodes are not a {h} x {w} grid")
    return v.reshape(v.shape[:-1] + (h, w))


def edge_images(values, h: int, w: int):
    """An edge map [.., n_edges] of the h x w grid graph (canonical edge ids) as two images:
    (horizontal [.., h, w - 1]: edge (i, j)-(i, j + 1); vertical [.., h - 1, w]: edge
    (i, j)-(i + 1, j))."""
    v = np.asarray(values)
    if v.shape[-1] != h * (w - 1) + (h - 1) * w:
        raise ValueError(f"{v.shape[-1]} edges are not those of a {h} x {w} grid")
    # canonical order: node by node, right neighbour before the one below
    hid = np.full((h, w - 1), -1, np.int64)
    vid = np.full((h - 1, w), -1, np.int64)
    e = 0
    for i in range(h):
        for j in range(w):
            if j < w - 1:
                hid[i, j] = e
                e += 1
            if i < h - 1:
                vid[i, j] = e
                e += 1
    return v[..., hid], v[..., vid]
