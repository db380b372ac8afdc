"""numpy restatement of the node co-assignment step (fw_chains_coassign_async): per group,
together = sum over districts d of A_d^T A_d with A_d = (labels[members][:, nodes] == d), and
cnt = the members.  A group is a rung under a ladder (every set has one chain on it), else all
chains."""
import numpy as np


def coassign(labels, k, nodes=None, rungs=None, n_groups=1):
    """{"together": uint64 [n_groups, m, m], "cnt": uint64 [n_groups]} of the plans ``labels``
    [n_chains, n] for the list ``nodes`` (None: all), in the list's order."""
    lab = np.asarray(labels)
    cols = lab if nodes is None else lab[:, np.asarray(nodes, np.int64)]
    m = cols.shape[1]
    together = np.zeros((n_groups, m, m), np.uint64)
    cnt = np.zeros(n_groups, np.uint64)
    for g in range(n_groups):
        members = cols if rungs is None else cols[np.asarray(rungs) == g]
        cnt[g] = members.shape[0]
        for d in range(k):
            a = (members == d).astype(np.float64)  # exact: counts stay far below 2^53
            together[g] += (a.T @ a).astype(np.uint64)
    return {"together": together, "cnt": cnt}


def add(a, b):
    return b if a is None else {key: a[key] + b[key] for key in a}
