"""CPU restatement of replica exchange across a base ladder (fw_chains_set_ladder /
fw_chains_exchange_async, include/flipwalk.h), built only from the oracle: ``run_chain``
segments with the stats carried over, ``philox4x32_10``, ``orc_u53`` and ``log1p``.

``exchange_ref`` is the swap rule on one replica set in Python floats; ``LadderRef`` keeps
the chains, their rungs and the rung stats (delta since the snapshot, then add) the way the
handle does; ``tempered_ref`` alternates run segments and exchanges.
"""
from __future__ import annotations

import numpy as np

from flipcomplexityempirical_amd._lib import RUNG_STATS_DTYPE
from flipcomplexityempirical_amd.chain import metropolis_table
from oracle import oracle as O

SNAP_FIELDS = ("yields", "steps", "accepts", "sum_cut", "sum_bnodes", "sum_invb")


def exchange_counter(round, r, g):
    """Philox counter of the pair (r, r+1) of the set whose smallest global chain id is g."""
    return (round & 0xFFFFFFFF, (1 << 30) | r, g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF)


def exchange_draw(seed, round, r, g):
    x = O.philox4x32_10(exchange_counter(round, r, g), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return O.lib().orc_u53(int(x[2]), int(x[3]))


def exchange_ref(cut, stuck, log_base, seed, round, g):
    """One exchange step of one replica set: cut[r] / stuck[r] belong to the chain on rung r.
    Returns (tried, done), bool [n_rungs], for the pairs (r, r+1) kept at r; the caller lets
    the chains of every done pair trade rungs."""
    n = len(cut)
    tried, done = np.zeros(n, bool), np.zeros(n, bool)
    for r in range(round & 1, n - 1, 2):
        if stuck[r] or stuck[r + 1]:
            continue
        d = int(cut[r]) - int(cut[r + 1])
        x = float(d) * (float(log_base[r]) - float(log_base[r + 1]))
        tried[r] = True
        done[r] = O.log1p(-exchange_draw(seed, round, r, g)) <= x
    return tried, done


class LadderRef:
    def __init__(self, graph, init, k, mode, bounds, bases, set_of_chain, rung_of_chain, seed,
                 chain_id0, log_base=None):
        import math
        self.g, self.k, self.mode, self.bounds = graph, k, mode, bounds
        self.seed, self.id0 = seed, chain_id0
        self.bases = [float(b) for b in bases]
        self.rows = [metropolis_table(b, graph.maxdeg) for b in self.bases]
        self.log_base = [math.log(b) for b in self.bases] if log_base is None else log_base
        self.set_of = np.asarray(set_of_chain, np.int64)
        self.rung = np.array(rung_of_chain, np.int32)
        C, R = len(self.rung), len(self.bases)
        self.chain_of = np.full((C // R, R), -1, np.int64)
        self.chain_of[self.set_of, self.rung] = np.arange(C)
        assert (self.chain_of >= 0).all()
        init = np.asarray(init, np.int16)
        self.labels = [init[c].copy() if init.ndim == 2 else init.copy() for c in range(C)]
        self.stats = [O.new_stats(1) for _ in range(C)]
        self.pops = [None] * C
        self.hc = np.zeros(graph.n_edges + 1, np.uint64)
        self.hb = np.zeros(graph.n + 1, np.uint64)
        self.rstats = np.zeros((C // R, R), RUNG_STATS_DTYPE)
        self.snapshot()

    def snapshot(self):
        self.snap = [{f: s[0][f] for f in SNAP_FIELDS} for s in self.stats]

    def run(self, steps):
        lo, hi = self.bounds
        for c in range(len(self.rung)):
            self.labels[c], self.stats[c], self.pops[c], _ = O.run_chain(
                self.g, self.labels[c], self.k, self.mode, lo, hi, self.rows[self.rung[c]],
                self.seed, self.id0 + c, steps, stats=self.stats[c], hist_cut=self.hc,
                hist_b=self.hb)

    def exchange(self, round):
        for s in range(self.chain_of.shape[0]):
            chains = self.chain_of[s].copy()
            for r, c in enumerate(chains):  # accumulate: delta since the snapshot, then add
                st, sn, rs = self.stats[c][0], self.snap[c], self.rstats[s, r]
                for f in SNAP_FIELDS:
                    if f == "sum_invb":
                        rs[f] = np.float64(rs[f]) + (np.float64(st[f]) - np.float64(sn[f]))
                    else:
                        rs[f] = rs[f] + (st[f] - sn[f])
                    sn[f] = st[f]
            cut = [self.stats[c][0]["cut"] for c in chains]
            stuck = [self.stats[c][0]["stuck"] for c in chains]
            g = self.id0 + int(chains.min())
            tried, done = exchange_ref(cut, stuck, self.log_base, self.seed, round, g)
            self.rstats[s]["swap_tried"] += tried
            self.rstats[s]["swap_done"] += done
            for r in np.flatnonzero(done):
                a, b = chains[r], chains[r + 1]
                self.chain_of[s, r], self.chain_of[s, r + 1] = b, a
                self.rung[a], self.rung[b] = r + 1, r

    def reset_observables(self):
        for s in self.stats:
            for f in ("yields", "sum_cut", "sum_bnodes"):
                s[0][f] = 0
            s[0]["sum_invb"] = 0.0
        self.hc[:] = 0
        self.hb[:] = 0
        self.rstats[...] = np.zeros((), RUNG_STATS_DTYPE)
        self.snapshot()

    def result(self):
        return {"labels": np.stack(self.labels), "stats": np.array([s[0] for s in self.stats]),
                "pops": np.stack(self.pops), "hist_cut": self.hc.copy(), "hist_b": self.hb.copy(),
                "rungs": self.rung.copy(), "rung_stats": self.rstats.copy()}


def tempered_ref(graph, init, k, mode, bounds, bases, set_of_chain, rung_of_chain, seed,
                 chain_id0, steps_per_round, n_rounds, round0=0):
    """n_rounds x (steps_per_round oracle steps of every chain under the bounds of its
    current rung, one exchange); rounds numbered from round0.  Returns LadderRef.result()."""
    ref = LadderRef(graph, init, k, mode, bounds, bases, set_of_chain, rung_of_chain, seed,
                    chain_id0)
    for i in range(n_rounds):
        ref.run(steps_per_round)
        ref.exchange(round0 + i)
    return ref.result()
