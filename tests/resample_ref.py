"""Restatement in Python integers of resampling plans across chains (fw_chains_clone_async /
fw_chains_resample_async, include/flipwalk.h).

``resample_map`` maps (cut, q, sign, u) to (W, T, S2, cref, offspring, src) exactly as the header
states it, with arbitrary-precision integers where the device carries limbs; ``draw_u`` is the one
Philox block of a round, from the oracle's Philox (the helper the ladder reference uses);
``gather`` applies a map to the arrays of a handle the way the clone moves them.
"""
from __future__ import annotations

import numpy as np

PLAN_FIELDS = ("cut", "bnodes", "npairs", "stuck")


def draw_u(seed, round, chain_id0):
    """u = x0 of the block key = seed, ctr = (lo32(round), 2^30 | 2^29, lo32(id0), hi32(id0))."""
    from oracle import oracle as O
    g = chain_id0 & (2**64 - 1)
    ctr = (round & 0xFFFFFFFF, (1 << 30) | (1 << 29), g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF)
    return int(O.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0])


def points(u, T, C):
    """p_j = floor(((j 2^32 + u) T) / (C 2^32)), j = 0..C-1."""
    return [(((j << 32) + u) * T) // (C << 32) for j in range(C)]


def resample_map(cut, q, sign, u):
    """One systematic resampling: returns a dict with W (uint32 [C]), T, S2, cref, offspring
    (int64 [C]), src (int32 [C]), survivors and max_offspring."""
    cut = [int(x) for x in cut]
    q = [int(x) for x in q]
    C = len(cut)
    assert sign in (1, -1) and q[0] == 1 << 30 and C >= 1
    cref = min(cut) if sign == 1 else max(cut)
    W = [q[sign * (x - cref)] for x in cut]
    cum, tot = [], 0
    for w in W:
        tot += w
        cum.append(tot)
    T = tot
    S2 = sum((w >> 10) ** 2 for w in W)
    # offspring: points are ascending, so one merge pass counts #{j : cum[i-1] <= p_j < cum[i]}
    n = [0] * C
    i = 0
    for p in points(u, T, C):
        while p >= cum[i]:
            i += 1
        n[i] += 1
    # dead chains in ascending index take the extra copies in ascending survivor index
    extras = [s for s in range(C) for _ in range(n[s] - 1)]
    dead = [i for i in range(C) if n[i] == 0]
    assert len(extras) == len(dead)
    src = list(range(C))
    for i, s in zip(dead, extras):
        src[i] = s
    return {"W": np.array(W, np.uint32), "T": T, "S2": S2, "cref": cref,
            "offspring": np.array(n, np.int64), "src": np.array(src, np.int32),
            "survivors": C - len(dead), "max_offspring": max(n)}


def gather(src, labels, stats, pops=None, waits=None, families=None):
    """What a clone with the map src leaves: the plan moves (labels, pops, the four plan fields
    of the stats records, the current wait draw, the family), the chain stays.  Returns new
    arrays in the order given (None where none was given)."""
    src = np.asarray(src, np.int64)
    assert np.array_equal(src[src], src), "sources must be fixed points"
    lab = np.asarray(labels)[src].copy()
    st = np.array(stats, copy=True)
    for f in PLAN_FIELDS:
        st[f] = np.asarray(stats)[f][src]
    out = [lab, st]
    out.append(None if pops is None else np.asarray(pops)[src].copy())
    if waits is None:
        out.append(None)
    else:
        w = np.array(waits, copy=True)
        w[:, 1] = np.asarray(waits)[src, 1]
        out.append(w)
    out.append(None if families is None else np.asarray(families)[src].copy())
    return out
