"""Host restatement of the district tallies (include/flipwalk.h, fw_chains_tally_async): exact
integer sums from int16 plans, strict wins and ties, and the seat histogram by group.  The GPU
tests compare with ``np.array_equal``: every result is an integer."""
from __future__ import annotations

import numpy as np


def sums(labels: np.ndarray, cols: np.ndarray, k: int) -> np.ndarray:
    """T[c][j][d] = sum of cols[j] over the nodes chain c labels d; int64 [C, n_cols, k]."""
    labels = np.asarray(labels)
    cols = np.atleast_2d(np.asarray(cols, np.int64))
    C, n = labels.shape
    out = np.zeros((C, cols.shape[0], k), np.int64)
    rows = np.repeat(np.arange(C), n)
    flat = labels.astype(np.int64).ravel()
    for j in range(cols.shape[0]):
        np.add.at(out[:, j, :], (rows, flat), np.tile(cols[j], C))
    return out


def seats(T: np.ndarray, elections) -> np.ndarray:
    """{wins, ties} of every election (a, b): int32 [C, n_el, 2]; a win is strict."""
    el = np.asarray(elections, np.int64).reshape(-1, 2)
    out = np.zeros((T.shape[0], len(el), 2), np.int32)
    for e, (a, b) in enumerate(el):
        out[:, e, 0] = (T[:, a, :] > T[:, b, :]).sum(axis=1)
        out[:, e, 1] = (T[:, a, :] == T[:, b, :]).sum(axis=1)
    return out


def seat_hist(S: np.ndarray, k: int, groups=None, n_groups: int = 1) -> np.ndarray:
    """hist[g][e][wins] = chains of group g whose election e gives ``wins`` seats; uint64
    [n_groups, n_el, k + 1].  ``groups`` [C] (default: all 0)."""
    C, n_el = S.shape[0], S.shape[1]
    g = np.zeros(C, np.int64) if groups is None else np.asarray(groups, np.int64)
    out = np.zeros((n_groups, n_el, k + 1), np.uint64)
    for e in range(n_el):
        np.add.at(out[:, e, :], (g, S[:, e, 0].astype(np.int64)), np.uint64(1))
    return out


def tally(labels, cols, k, elections=(), groups=None, n_groups: int = 1):
    """(sums, seats, one tally's histogram) of the plans ``labels``."""
    T = sums(labels, cols, k)
    S = seats(T, elections)
    return T, S, seat_hist(S, k, groups, n_groups)
