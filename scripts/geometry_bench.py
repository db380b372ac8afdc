#!/usr/bin/env python3
"""Cost of a per-district geometry measurement (Chains.geometry) at the bench shapes, one JSON
line per measurement (raw lines are kept under profiles/geometry/).

  shape c3 / c4   after --steps steps: 5 x (geometry; sync) under a host clock that ends in the
                  synchronise (the handle's stream is the library's own, so the figure holds
                  one launch's latency as well), 20 measurements enqueued back to back over one
                  synchronise, a device-to-device copy of n_chains x label bytes under HIP
                  events, and the host route: labels() plus tests/geometry_ref.py over
                  --host-chains chains, scaled to all of them; with edge weights, areas and
                  exteriors set, and the burst again with all three left out
  sampled (c2)    50 x (run_async(100), record) around one sync, with and without a measurement
                  per launch, 8 interleaved repeats on one handle

    python scripts/geometry_bench.py [--only c3|c4|sampled] [--steps N] [--chains C]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import geometry_ref  # noqa: E402
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
    arrays = (rng.integers(0, 1000, w.graph.n_edges).astype(np.int64),
              rng.integers(0, 1000, w.graph.n).astype(np.int64),
              rng.integers(0, 1000, w.graph.n).astype(np.int64))
    ch.set_geometry(*arrays)
    return w, ch, arrays


def burst_ms(ch, n=20):
    t0 = time.perf_counter()
    for _ in range(n):
        ch.geometry()
    ch.sync()
    return (time.perf_counter() - t0) * 1e3 / n


def shape(name, steps, chains, host_chains):
    import torch
    w, ch, arrays = make(name, chains)
    ch.run(steps)
    ch.geometry()
    ch.sync()  # warm: code object loaded
    bits = ch.geometry_info()["label_bits"]
    single = []
    for _ in range(5):
        t0 = time.perf_counter()
        ch.geometry()
        ch.sync()
        single.append((time.perf_counter() - t0) * 1e3)
    burst = burst_ms(ch)
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
    edges = w.graph.edges()
    t0 = time.perf_counter()
    G = np.concatenate([geometry_ref.districts(labels[c:c + 256], edges, w.k, *arrays)
                        for c in range(0, hc, 256)])
    t_ref = (time.perf_counter() - t0) * 1e3 * ch.n_chains / hc
    assert np.array_equal(G, ch.district_geometry()[:hc])
    # the same with unit weights, unit areas and no exterior: no weight array is staged
    ch.set_geometry()
    ch.geometry()
    ch.sync()
    burst_unit = burst_ms(ch)
    # algorithmic L2 traffic of one measurement: every chain's label words once, and per
    # workgroup of 16 chains the edge list {u, w, weight} and the two node arrays once
    E, n = w.graph.n_edges, w.graph.n
    lab_words = ((n * bits + 31) // 32 + 1 + 3) & ~3
    groups = -(-ch.n_chains // 16)
    traffic = ch.n_chains * lab_words * 4 + groups * (E * 12 + n * 8) + ch.n_chains * w.k * 40
    emit(what="geometry", shape=name, chains=ch.n_chains, nodes=n, edges=E, k=w.k, label_bits=bits,
         steps=steps, geometry_sync_ms=single, geometry_burst_ms=burst,
         geometry_burst_unit_ms=burst_unit, label_bytes=ch.n_chains * lab_bytes,
         d2d_copy_ms=copies, host_labels_ms=t_labels, host_ref_ms_scaled=t_ref,
         host_ref_chains=hc, algorithmic_l2_bytes=traffic,
         ratio_to_copy=burst / min(copies), host_over_geometry=(t_labels + t_ref) / burst)
    ch.close()


def sampled(repeats):
    w, ch, _ = make("c2")
    ch.enable_series(50 * 2 * repeats + 200)
    ch.run(1000)
    ch.run_sampled(100, 50, geometry=True)  # warm both loops
    plain, measured = [], []
    for _ in range(repeats):
        for out, flag in ((plain, False), (measured, True)):
            t0 = time.perf_counter()
            ch.run_sampled(100, 50, geometry=flag)
            out.append((time.perf_counter() - t0) * 1e3)
    emit(what="sampled", shape="c2", chains=ch.n_chains, loop="50 x (run_async(100), record)",
         plain_ms=plain, with_geometry_ms=measured, plain_spread_ms=max(plain) - min(plain),
         mean_difference_ms=float(np.mean(measured) - np.mean(plain)))
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
