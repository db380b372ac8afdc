"""What the pairwise plan distances of an ensemble are read for (numpy only): distinct plans,
medoids, the mean distance, a Euclidean embedding, a two-sample statistic between two groups
of chains and landmark assignment.  The inputs are ``Chains.distance_matrix()``,
``distance_rowsums()`` and ``pair_distance_hist()``; nothing here touches the device.
"""
from __future__ import annotations

import numpy as np


def _square(D) -> np.ndarray:
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError(f"a square distance matrix is expected, got shape {D.shape}")
    return D


def distinct_plans(D):
    """Classes of positions at distance 0 of a symmetric matrix: (``cls`` int64 [m], the lowest
    position of each position's class; the number of classes).  Distance 0 between plans is an
    equivalence, so one pass over the rows suffices."""
    D = _square(D)
    m = D.shape[0]
    cls = np.full(m, -1, np.int64)
    for i in range(m):
        if cls[i] < 0:
            same = (D[i] == 0) & (cls < 0)
            same[i] = True
            cls[same] = i
    return cls, int(np.unique(cls).size)


def medoid(rowsums) -> int:
    """The position with the least summed distance to all others (the lowest on ties)."""
    rowsums = np.asarray(rowsums).ravel()
    if rowsums.size < 1:
        raise ValueError("medoid of no rows")
    return int(np.argmin(rowsums))


def mean_pairwise(hist) -> float:
    """The mean of the distances counted in a histogram (``pair_distance_hist``): nan when it
    is empty."""
    hist = np.asarray(hist, np.float64).ravel()
    total = hist.sum()
    if total == 0:
        return float("nan")
    return float((hist * np.arange(hist.size)).sum() / total)


def classical_mds(D, dims: int = 2):
    """Classical (Torgerson) scaling of a symmetric distance matrix: B = -1/2 J D^2 J with the
    centring J, its ``dims`` largest eigenpairs; returns (coordinates float64 [m, dims], the
    eigenvalues float64 [dims]).  Negative eigenvalues (Hamming distances between plans are a
    metric but not Euclidean in general) contribute zero coordinates."""
    D = _square(D).astype(np.float64)
    m = D.shape[0]
    dims = int(dims)
    if dims < 1 or dims > m:
        raise ValueError(f"dims = {dims} outside [1, {m}]")
    J = np.eye(m) - 1.0 / m
    B = -0.5 * J @ (D * D) @ J
    w, V = np.linalg.eigh((B + B.T) / 2)
    order = np.argsort(w)[::-1][:dims]
    w, V = w[order], V[:, order]
    return V * np.sqrt(np.maximum(w, 0.0)), w


def energy_distance(D_ab, D_aa, D_bb) -> float:
    """The energy distance between two groups of plans, 2 E d(A, B) - E d(A, A') - E d(B, B'),
    from the rectangular matrix between the groups and the symmetric matrix of each (V-statistic
    form: the within-group means include the zero diagonal); 0 for identical groups, and
    non-negative whenever the distance is of negative type."""
    D_ab = np.asarray(D_ab, np.float64)
    D_aa, D_bb = _square(D_aa).astype(np.float64), _square(D_bb).astype(np.float64)
    if D_ab.shape != (D_aa.shape[0], D_bb.shape[0]):
        raise ValueError(f"D_ab has shape {D_ab.shape}, the groups have {D_aa.shape[0]} and "
                         f"{D_bb.shape[0]} members")
    return float(2.0 * D_ab.mean() - D_aa.mean() - D_bb.mean())


def landmark_assign(D):
    """Per row of a rectangular matrix (rows: plans, columns: landmarks) the nearest landmark
    (the lowest on ties) and its distance: (int64 [ma], D's dtype [ma])."""
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[1] < 1:
        raise ValueError(f"a matrix [plans, landmarks] is expected, got shape {D.shape}")
    j = np.argmin(D, axis=1)
    return j.astype(np.int64), D[np.arange(D.shape[0]), j]
