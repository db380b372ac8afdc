"""Host restatement of the per-district geometry (include/flipwalk.h,
fw_chains_geometry_async): exact int64 counts and sums from int16 plans, ``Graph.edges()`` and
the three arrays, and the histogram of the per-district cut by group.  The GPU tests compare
with ``np.array_equal``: every result is an integer."""
from __future__ import annotations

import numpy as np


def districts(labels, edges, k: int, edge_weights=None, area=None, exterior=None) -> np.ndarray:
    """G[c][d] = {nodes, cut edges, interior perimeter, exterior perimeter, area} of district d
    of plan c; int64 [C, k, 5].  None: unit edge weights, unit areas, no exterior."""
    lab = np.asarray(labels).astype(np.int64)
    C, n = lab.shape
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.ones(len(e), np.int64) if edge_weights is None else np.asarray(edge_weights, np.int64)
    a = np.ones(n, np.int64) if area is None else np.asarray(area, np.int64)
    x = np.zeros(n, np.int64) if exterior is None else np.asarray(exterior, np.int64)
    out = np.zeros((C, k, 5), np.int64)
    rows = np.repeat(np.arange(C), n)
    flat = lab.ravel()
    np.add.at(out[:, :, 0], (rows, flat), 1)
    np.add.at(out[:, :, 3], (rows, flat), np.tile(x, C))
    np.add.at(out[:, :, 4], (rows, flat), np.tile(a, C))
    lu, lw = lab[:, e[:, 0]], lab[:, e[:, 1]]  # [C, E]
    c_idx, e_idx = np.nonzero(lu != lw)
    for side in (lu, lw):
        np.add.at(out[:, :, 1], (c_idx, side[c_idx, e_idx]), 1)
        np.add.at(out[:, :, 2], (c_idx, side[c_idx, e_idx]), w[e_idx])
    return out


def cut_hist(G, n_edges: int, groups=None, n_groups: int = 1) -> np.ndarray:
    """hist[g][cut] = districts of the chains of group g with ``cut`` cut edges, one
    measurement; uint64 [n_groups, n_edges + 1].  ``groups`` [C] (default: all 0)."""
    G = np.asarray(G)
    C, k = G.shape[0], G.shape[1]
    g = np.zeros(C, np.int64) if groups is None else np.asarray(groups, np.int64)
    out = np.zeros((n_groups, n_edges + 1), np.uint64)
    np.add.at(out, (np.repeat(g, k), G[:, :, 1].ravel()), np.uint64(1))
    return out
