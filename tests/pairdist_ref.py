"""Host restatement of the pairwise plan distances (include/flipwalk.h,
fw_chains_pairdist_async): exact integer counts from int16 plans.  The GPU tests compare with
it."""
import numpy as np


def matrix(X, a, b=None, block=64):
    """int32 [ma, mb]: D[i, j] = #{v : X[a[i], v] != X[b[j], v]} of plans ``X`` [n_chains, n];
    ``b=None`` means ``b = a``.  Done in row blocks so the boolean cube stays small."""
    X = np.asarray(X)
    a = np.asarray(a, np.int64)
    b = a if b is None else np.asarray(b, np.int64)
    Xb = X[b]
    D = np.empty((len(a), len(b)), np.int32)
    for i0 in range(0, len(a), block):
        Xa = X[a[i0:i0 + block]]
        D[i0:i0 + block] = (Xa[:, None, :] != Xb[None, :, :]).sum(-1)
    return D


def rowsum(D):
    """int64 [ma]"""
    return np.asarray(D, np.int64).sum(axis=1)


def nearest(D, symmetric):
    """int32 [ma, 2]: (the least value of row i, the lowest j attaining it); in the symmetric
    case position j = i is left out, and a single member gives (-1, -1)."""
    D = np.asarray(D, np.int64)
    ma, mb = D.shape
    out = np.full((ma, 2), -1, np.int32)
    for i in range(ma):
        row = D[i].copy()
        if symmetric:
            if mb == 1:
                continue
            row[i] = np.iinfo(np.int64).max
        j = int(np.argmin(row))  # the first of equal values
        out[i] = (row[j], j)
    return out


def hist(D, n, symmetric):
    """uint64 [n + 1]: counts of the values of D; over positions i < j in the symmetric case."""
    D = np.asarray(D, np.int64)
    vals = D[np.triu_indices(D.shape[0], 1)] if symmetric else D.ravel()
    return np.bincount(vals, minlength=n + 1).astype(np.uint64)


def measure(X, n, a, b=None):
    """(D, rowsum, nearest, hist) of one measurement."""
    D = matrix(X, a, b)
    return D, rowsum(D), nearest(D, b is None), hist(D, n, b is None)
