#!/usr/bin/env python3
"""Cost of a district tally (Chains.tally) at the bench shapes, one JSON line per measurement
(raw lines are kept under profiles/tally/).

  shape c3 / c4   after --steps steps: 5 x (tally; sync) under a host clock that ends in the
                  synchronise (the handle's stream is the library's own, so the figure holds
                  one launch's latency as well), 20 tallies enqueued back to back over one
                  synchronise, a device-to-device copy of n_chains x label bytes under HIP
                  events, and the host route: labels() plus a numpy bincount over --host-chains
                  chains, scaled to all of them
  sampled (c2)    50 x (run_async(100), record) around one sync, with and without a tally per
                  launch, 8 interleaved repeats on one handle

    python scripts/tally_bench.py [--only c3|c4|sampled] [--steps N] [--chains C]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds  # noqa: E402
from flipcomplexityempirical_amd.workloads import workload  # noqa: E402


def emit(**kw):
    kw["build"] = _lib.build_info()
    print(json.dumps(kw), flush=True)


def make(name, chains=None):
    w = workload(name)
    n_chains = chains or w.chains
    dg = DeviceGraph(w.graph)
    ch = Chains(dg, n_chains, w.k, w.init, proposal=w.proposal,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent), base=w.base, seed=0)
    rng = np.random.default_rng(0)
    cols = rng.integers(0, 100, (2, w.graph.n)).astype(np.int64)
    ch.set_columns({"pink": cols[0], "purple": cols[1]})
    ch.set_elections([("pink", "purple")])
    return w, ch, cols


def host_sums(labels, cols, k):
    C, n = labels.shape
    idx = (np.arange(C, dtype=np.int64)[:, None] * k + labels).ravel()
    return np.stack([np.bincount(idx, np.tile(c, C), C * k).reshape(C, k) for c in cols],
                    axis=1).astype(np.int64)


def shape(name, steps, chains, host_chains):
    import torch
    w, ch, cols = make(name, chains)
    ch.run(steps)
    ch.tally()
    ch.sync()  # warm: code object loaded
    bits = ch.tally_info()["label_bits"]
    single = []
    for _ in range(5):
        t0 = time.perf_counter()
        ch.tally()
        ch.sync()
        single.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for _ in range(20):
        ch.tally()
    ch.sync()
    burst = (time.perf_counter() - t0) * 1e3 / 20
    lab_bytes = (((w.graph.n * bits + 7) // 8 + 8) + 15) // 16 * 16
    src = torch.zeros(ch.n_chains * lab_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    copies = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    labels = ch.labels()
    t_labels = (time.perf_counter() - t0) * 1e3
    hc = min(host_chains, ch.n_chains)
    t0 = time.perf_counter()
    T = host_sums(labels[:hc], cols, w.k)
    t_sums = (time.perf_counter() - t0) * 1e3 * ch.n_chains / hc
    assert np.array_equal(T, ch.tallies()[:hc])
    emit(what="tally", shape=name, chains=ch.n_chains, nodes=w.graph.n, k=w.k, label_bits=bits,
         steps=steps, n_cols=2, n_elections=1, tally_sync_ms=single, tally_burst_ms=burst,
         label_bytes=ch.n_chains * lab_bytes, d2d_copy_ms=copies, host_labels_ms=t_labels,
         host_sums_ms_scaled=t_sums, host_sums_chains=hc,
         ratio_to_copy=burst / min(copies), host_over_tally=(t_labels + t_sums) / burst)
    ch.close()


def sampled(repeats):
    w, ch, _ = make("c2")
    ch.enable_series(50 * 2 * repeats + 200)
    ch.run(1000)
    ch.run_sampled(100, 50, tally=True)  # warm both loops
    plain, tallied = [], []
    for _ in range(repeats):
        for out, flag in ((plain, False), (tallied, True)):
            t0 = time.perf_counter()
            ch.run_sampled(100, 50, tally=flag)
            out.append((time.perf_counter() - t0) * 1e3)
    emit(what="sampled", shape="c2", chains=ch.n_chains, loop="50 x (run_async(100), record)",
         plain_ms=plain, with_tally_ms=tallied,
         plain_spread_ms=max(plain) - min(plain), mean_difference_ms=float(np.mean(tallied) - np.mean(plain)))
    ch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c3", "c4", "sampled"])
    ap.add_argument("--steps", type=int, default=25000)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--host-chains", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=8)
    a = ap.parse_args()
    for name in ("c3", "c4"):
        if a.only in (None, name):
            shape(name, a.steps, a.chains, a.host_chains)
    if a.only in (None, "sampled"):
        sampled(a.repeats)
