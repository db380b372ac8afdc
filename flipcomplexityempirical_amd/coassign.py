"""Scores of the node co-assignment matrix (``Chains.coassignment()``, ``coassign_counts()``).

Pure numpy on the integer arrays the device accumulates: ``together`` is uint64 [n_groups, m, m]
(or [m, m] for one group), how many plans of a group put nodes i and j of the list in one
district, and ``cnt`` uint64 [n_groups] (or a scalar), the plans counted.  Nothing here touches
a GPU.
"""
from __future__ import annotations

import numpy as np


def _shape(together, cnt):
    """float64 together [g, m, m], float64 cnt [g, 1, 1], and whether the caller gave one group."""
    t = np.asarray(together)
    single = t.ndim == 2
    if single:
        t = t[None]
    if t.ndim != 3 or t.shape[1] != t.shape[2]:
        raise ValueError(f"together must be [n_groups, m, m] or [m, m], got {np.shape(together)}")
    c = np.asarray(cnt, np.float64).reshape(-1)
    if c.size != t.shape[0]:
        raise ValueError(f"cnt has {c.size} groups, together {t.shape[0]}")
    if (c <= 0).any():
        raise ValueError("a group has no counted plans")
    return t.astype(np.float64), c[:, None, None], single


def frequency(together, cnt) -> np.ndarray:
    """The fraction of plans that put i and j together: float64, the shape of ``together``."""
    t, c, single = _shape(together, cnt)
    f = t / c
    return f[0] if single else f


def separation(together, cnt) -> np.ndarray:
    """1 - frequency: the fraction of plans that separate i and j, a pseudo-metric on the nodes
    (symmetric, zero on the diagonal, and a plan that separates i from k separates i from j or
    j from k)."""
    return 1.0 - frequency(together, cnt)


def expected_mates(together, cnt) -> np.ndarray:
    """float64 [n_groups, m] (or [m]): the mean number of listed nodes, itself included, that
    share node i's district: row sums over cnt."""
    t, c, single = _shape(together, cnt)
    e = t.sum(axis=2) / c[:, :, 0]
    return e[0] if single else e


def pair_entropy(together, cnt) -> np.ndarray:
    """The entropy, in bits, of the event "i and j share a district" per pair: 0 where the pair
    is always or never together, 1 where it is a coin flip.  The shape of ``together``."""
    f = frequency(together, cnt)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -(np.where(f > 0, f * np.log2(f), 0.0) + np.where(f < 1, (1 - f) * np.log2(1 - f), 0.0))
    return h + 0.0  # no negative zeros


def edge_cut_from_coassign(together, cnt, pairs) -> np.ndarray:
    """uint64 [n_groups, len(pairs)] (or [len(pairs)]): plans that separate the list positions
    ``pairs[:, 0]`` and ``pairs[:, 1]``: cnt - together.  With all nodes listed and the graph's
    canonical edges as pairs this is the census's edge-cut count."""
    t = np.asarray(together)
    single = t.ndim == 2
    if single:
        t = t[None]
    c = np.asarray(cnt, np.uint64).reshape(-1)
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = c[:, None] - t[:, p[:, 0], p[:, 1]].astype(np.uint64)
    return out[0] if single else out


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def cores(together, cnt, threshold: float, edges=None) -> np.ndarray:
    """int64 [n_groups, m] (or [m]): a core label per node.  Cores are the connected components
    of the pairs (i, j) with frequency >= ``threshold``, over all pairs, or with ``edges`` (list
    positions, [E, 2]) only along those; by union-find.  Labels are 0, 1, .. in the order of
    each core's lowest position."""
    f = frequency(together, cnt)
    single = f.ndim == 2
    if single:
        f = f[None]
    m = f.shape[1]
    e = None if edges is None else np.asarray(edges, np.int64).reshape(-1, 2)
    out = np.empty((f.shape[0], m), np.int64)
    for g in range(f.shape[0]):
        if e is None:
            iu, ju = np.nonzero(np.triu(f[g] >= threshold, 1))
        else:
            keep = f[g][e[:, 0], e[:, 1]] >= threshold
            iu, ju = e[keep, 0], e[keep, 1]
        parent = list(range(m))
        for a, b in zip(iu.tolist(), ju.tolist()):
            ra, rb = _find(parent, a), _find(parent, b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        roots = np.array([_find(parent, x) for x in range(m)], np.int64)
        _, out[g] = np.unique(roots, return_inverse=True)  # roots are lowest positions
    return out[0] if single else out
