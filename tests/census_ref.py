"""numpy restatement of the ensemble census (fw_chains_census_async): from the plans ``labels``
int [n_chains, n] and, under a ladder, the chains' rungs, the counts one census adds.  Shared by
test_gpu_census.py, test_census_host.py and scripts/census_time.py."""
import numpy as np


def census(graph, labels, k, rungs=None, n_groups=1):
    """{"cnt": uint64 [n_groups], "occ": [n_groups, n, k], "ecut": [n_groups, n_edges], "bnd":
    [n_groups, n]} of the plans ``labels``; chain c counts under group rungs[c] (0 without)."""
    lab = np.asarray(labels, np.int64)
    C, n = lab.shape
    grp = np.zeros(C, np.int64) if rungs is None else np.asarray(rungs, np.int64)
    e = graph.edges().astype(np.int64)  # canonical order: pairs u < w in CSR row order
    src = np.repeat(np.arange(n), np.diff(graph.rowptr))
    cnt = np.zeros(n_groups, np.uint64)
    occ = np.zeros((n_groups, n, k), np.uint64)
    ecut = np.zeros((n_groups, len(e)), np.uint64)
    bnd = np.zeros((n_groups, n), np.uint64)
    for g in range(n_groups):
        X = lab[grp == g]
        cnt[g] = len(X)
        for d in range(k):
            occ[g, :, d] = (X == d).sum(axis=0)
        ecut[g] = (X[:, e[:, 0]] != X[:, e[:, 1]]).sum(axis=0)
        foreign = (X[:, src] != X[:, graph.col]).astype(np.int64)  # [chains, nnz]
        per_node = np.zeros((len(X), n), np.int64)
        if foreign.shape[1]:
            np.add.at(per_node, (slice(None), src), foreign)
        bnd[g] = (per_node > 0).sum(axis=0)
    return {"cnt": cnt, "occ": occ, "ecut": ecut, "bnd": bnd}


def add(total, one):
    """Accumulate one census into a running total (None: the first)."""
    return one if total is None else {key: total[key] + one[key] for key in one}


def census_loop(graph, labels, k, rungs=None, n_groups=1):
    """The same counts by a loop over chains and nodes (the check of ``census`` itself)."""
    n = graph.n
    edges = [(u, int(w)) for u in range(n) for w in graph.neighbors(u) if w > u]
    out = {"cnt": np.zeros(n_groups, np.uint64), "occ": np.zeros((n_groups, n, k), np.uint64),
           "ecut": np.zeros((n_groups, len(edges)), np.uint64),
           "bnd": np.zeros((n_groups, n), np.uint64)}
    for c, X in enumerate(np.asarray(labels)):
        g = 0 if rungs is None else int(rungs[c])
        out["cnt"][g] += 1
        for v in range(n):
            out["occ"][g, v, int(X[v])] += 1
            if any(X[int(w)] != X[v] for w in graph.neighbors(v)):
                out["bnd"][g, v] += 1
        for i, (u, w) in enumerate(edges):
            if X[u] != X[w]:
                out["ecut"][g, i] += 1
    return out
