"""numpy restatement of fw_chains_series_acf (include/flipwalk.h): the by-rung regroup, the
exact lagged sums and the pooled autocovariances, with the header's evaluation and reduction
order, so that the device output can be compared bit for bit.  A helper, not a test.

numpy's elementwise float64 ufuncs are single IEEE operations (no fused multiply-add across
two calls); the only ordered sum, over the members of a group, is written as a Python loop
over 256-wide rows and an explicit halving tree, never as numpy's own reduction."""
import numpy as np

POOL_WIDTH = 256


def regroup(x, rung, set_of_chain, n_rungs):
    """out[t][set_of_chain[c] * n_rungs + rung[t][c]] = x[t][c]."""
    x, rung = np.asarray(x), np.asarray(rung)
    slot = np.asarray(set_of_chain, np.int64)[None, :] * int(n_rungs) + rung
    out = np.full_like(x, -1)
    np.put_along_axis(out, slot, x, axis=1)
    return out


def lagged_sums(x, max_lag):
    """int64 [n_series][3][max_lag + 1] = {P, A, B} of the columns of x [n][n_series]."""
    x = np.asarray(x).astype(np.int64)
    n, N = x.shape
    out = np.zeros((N, 3, max_lag + 1), np.int64)
    for l in range(max_lag + 1):
        out[:, 0, l] = (x[:n - l] * x[l:]).sum(axis=0)
        out[:, 1, l] = x[:n - l].sum(axis=0)
        out[:, 2, l] = x[l:].sum(axis=0)
    return out


def terms(sums, n):
    """float64 [n_series][max_lag + 3]: c_j[0..max_lag], m_j, m_j^2, each evaluated in the
    header's order."""
    sums = np.asarray(sums, np.int64)
    N, _, L1 = sums.shape
    dn = np.float64(n)
    m = sums[:, 1, 0].astype(np.float64) / dn
    out = np.empty((N, L1 + 2), np.float64)
    for l in range(L1):
        P = sums[:, 0, l].astype(np.float64)
        ab = (sums[:, 1, l] + sums[:, 2, l]).astype(np.float64)
        out[:, l] = ((P - m * ab) + np.float64(n - l) * m * m) / dn
    out[:, L1] = m
    out[:, L1 + 1] = m * m
    return out


def ordered_sum(t):
    """The pooled sum of the rows of t [members][k]: partial p = the sequential sum from +0.0,
    in ascending position, of the members at positions p, p + 256, ..; then the halving tree."""
    t = np.asarray(t, np.float64)
    part = np.zeros((POOL_WIDTH, t.shape[1]), np.float64)
    for r0 in range(0, t.shape[0], POOL_WIDTH):
        row = t[r0:r0 + POOL_WIDTH]
        part[:row.shape[0]] = part[:row.shape[0]] + row
    h = POOL_WIDTH // 2
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0].copy()


def pooled(sums, n, n_rungs=0):
    """float64 [n_groups][max_lag + 3]: one group of every series (n_rungs == 0), or group r =
    the slots set * n_rungs + r in ascending set."""
    t = terms(sums, n)
    if not n_rungs:
        return ordered_sum(t)[None, :]
    return np.stack([ordered_sum(t[r::n_rungs]) for r in range(n_rungs)])


def series_acf(x, max_lag, n_rungs=0):
    """(per_series, pooled) of a window x [n][n_series] (already regrouped for by-rung)."""
    s = lagged_sums(x, max_lag)
    return s, pooled(s, np.asarray(x).shape[0], n_rungs)
