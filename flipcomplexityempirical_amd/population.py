"""Host side of resampling plans across chains (fw_chains_resample_async, include/flipwalk.h):
the integer weight table of a change of base, and what the resample's integer sums mean.

A population of chains stationary under cut_accept with base b (law f(x) * b ** (-cut(x)), f free
of the base) is turned into one for base b' by the importance weight r ** (-cut), r = b' / b.  The
device resamples by W_i = q[sign * (cut_i - cref)] with the heaviest chain at 2^30, so nothing
underflows wherever the population sits; the host forms the estimates below from the sums it
reads back.
"""
from __future__ import annotations

import math

import numpy as np

ONE = 1 << 30  # the heaviest chain's weight


def weight_table(base_from: float, base_to: float, n_edges: int):
    """(q, sign) of fw_chains_resample_async for the change of base base_from -> base_to:
    q[d] = round(2^30 * rho ** d), d = 0..n_edges, rho = min(r, 1 / r), r = base_to / base_from;
    sign = +1 if r > 1 (fewer cut edges weigh more: cref is the minimum) else -1.  q is uint32,
    non-increasing, q[0] == 2^30."""
    b0, b1 = float(base_from), float(base_to)
    if not (b0 > 0.0 and b1 > 0.0 and math.isfinite(b0) and math.isfinite(b1)):
        raise ValueError("bases must be positive and finite")
    if n_edges < 0:
        raise ValueError("n_edges must be >= 0")
    r = b1 / b0
    rho = min(r, 1.0 / r)
    q = np.rint(float(ONE) * np.power(rho, np.arange(int(n_edges) + 1, dtype=np.float64)))
    q = np.minimum.accumulate(q).astype(np.uint32)  # pow is monotone; rounding keeps it so
    q[0] = ONE
    return q, (1 if r > 1.0 else -1)


def _field(info, key, index):
    return int(info[key]) if isinstance(info, dict) else int(info[index])


def effective_sample_size(info) -> float:
    """(sum W)^2 / sum W^2 of the last resample from its integer sums, (T >> 10)^2 / S2
    (``Chains.resample_info()`` or the raw int64 [8])."""
    T, S2 = _field(info, "T", 2), _field(info, "S2", 3)
    if S2 <= 0:
        raise ValueError("nothing has been resampled")
    return float((T >> 10) ** 2) / float(S2)


def log_weight_mean(info, base_from: float, base_to: float, n_chains: int) -> float:
    """log of the population mean of r ** (-cut), r = base_to / base_from: log T - log C -
    30 log 2 - cref * log r.  The stage's free-energy increment log(Z(b') / Z(b)) as the
    population estimates it; ``Chains.run_annealed`` sums them."""
    T, cref = _field(info, "T", 2), _field(info, "cref", 4)
    if T <= 0:
        raise ValueError("nothing has been resampled")
    r = float(base_to) / float(base_from)
    return math.log(T) - math.log(int(n_chains)) - 30.0 * math.log(2.0) - cref * math.log(r)


def family_sizes(families) -> np.ndarray:
    """int64 [n_chains]: how many current plans descend from each chain's initial plan."""
    f = np.asarray(families)
    return np.bincount(f, minlength=len(f)).astype(np.int64)
