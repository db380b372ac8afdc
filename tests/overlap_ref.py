"""Host restatement of the plan overlap (include/flipwalk.h, fw_chains_overlap_async): exact
integer counts from int16 plans with ``np.bincount``.  The GPU tests compare with it."""
import numpy as np


def overlap(ref, cur, k):
    """(O int64 [n_chains, k, k], dist int32 [n_chains]) of current plans ``cur`` [n_chains, n]
    against ``ref``, [n] (shared) or [n_chains, n]: O[c, d, e] = #{v : ref_c(v) = d and
    cur_c(v) = e}, dist[c] = #{v : ref_c(v) != cur_c(v)}."""
    cur = np.asarray(cur, np.int64)
    ref = np.broadcast_to(np.asarray(ref, np.int64), cur.shape)
    C = cur.shape[0]
    O = np.empty((C, k, k), np.int64)
    for c in range(C):
        O[c] = np.bincount(ref[c] * k + cur[c], minlength=k * k).reshape(k, k)
    return O, (ref != cur).sum(axis=1).astype(np.int32)


def dist_hist(dist, n, groups=None, n_groups=1):
    """uint64 [n_groups, n + 1]: chains per distance, by ``groups`` [n_chains] (None: one)."""
    dist = np.asarray(dist, np.int64)
    g = np.zeros(len(dist), np.int64) if groups is None else np.asarray(groups, np.int64)
    return np.bincount(g * (n + 1) + dist, minlength=n_groups * (n + 1)).reshape(
        n_groups, n + 1).astype(np.uint64)
