#!/usr/bin/env python3
"""Cost of a plan-overlap measurement (Chains.overlap) at the bench shapes, one JSON line per
measurement (raw lines are kept under profiles/overlap/).

  shape c3 / c4   after --steps steps, against a snapshot reference taken 1,000 steps earlier
                  and against partners: 5 x (overlap; sync) under a host clock that ends in the
                  synchronise (the handle's stream is the library's own, so the figure holds one
                  launch's latency as well), 20 measurements enqueued back to back over one
                  synchronise, set_reference() alone (the snapshot copy), a device-to-device
                  copy of n_chains x label bytes under HIP events (the kernel reads twice that:
                  ratio_to_2x_copy), and the host route: labels() twice plus
                  tests/overlap_ref.py over --host-chains chains, scaled to all of them
  sampled (c2)    50 x (run_async(100), record) around one sync, with and without a measurement
                  per launch, 8 interleaved repeats on one handle

    python scripts/overlap_bench.py [--only c3|c4|sampled] [--steps N] [--chains C]
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

import overlap_ref  # noqa: E402
from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds  # noqa: E402
from flipcomplexityempirical_amd.workloads import workload  # noqa: E402


def emit(**kw):
    kw["build"] = _lib.build_info()
    print(json.dumps(kw), flush=True)


def make(name, chains=None):
    w = workload(name)
    dg = DeviceGraph(w.graph)
    ch = Chains(dg, chains or w.chains, w.k, w.init, proposal=w.proposal,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent), base=w.base, seed=0)
    return w, ch


def timed(ch, f, n=5):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ch.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def burst_ms(ch, against, n=20):
    t0 = time.perf_counter()
    for _ in range(n):
        ch.overlap(against)
    ch.sync()
    return (time.perf_counter() - t0) * 1e3 / n


def shape(name, steps, chains, host_chains):
    import torch
    w, ch = make(name, chains)
    ch.run(max(steps - 1000, 0))
    ch.set_reference()
    ch.set_partners()
    ch.run(min(steps, 1000))
    ch.overlap()
    ch.overlap("partner")
    ch.sync()  # warm: code object loaded
    bits = ch.overlap_info()["label_bits"]
    single = {a: timed(ch, lambda a=a: ch.overlap(a)) for a in ("reference", "partner")}
    burst = {a: burst_ms(ch, a) for a in ("reference", "partner")}
    lab_bytes = (w.graph.n * bits + 31) // 32 * 4
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
    # the host route: both plans read back, then the numpy reference on some of the chains
    ch.overlap()
    ref = ch.reference()
    t0 = time.perf_counter()
    labels = ch.labels()
    t_labels = 2 * (time.perf_counter() - t0) * 1e3
    hc = min(host_chains, ch.n_chains)
    t0 = time.perf_counter()
    O, dist = overlap_ref.overlap(ref[:hc], labels[:hc], w.k)
    t_ref = (time.perf_counter() - t0) * 1e3 * ch.n_chains / hc
    assert np.array_equal(O, ch.overlap_matrix()[:hc])
    assert np.array_equal(dist, ch.plan_distance()[:hc])
    snapshot = timed(ch, ch.set_reference)
    emit(what="overlap", shape=name, chains=ch.n_chains, nodes=w.graph.n, k=w.k, label_bits=bits,
         steps=steps, overlap_sync_ms=single, overlap_burst_ms=burst, set_reference_ms=snapshot,
         label_bytes=ch.n_chains * lab_bytes, d2d_copy_ms=copies, host_labels_ms=t_labels,
         host_ref_ms_scaled=t_ref, host_ref_chains=hc, mean_distance=float(dist.mean()),
         ratio_to_2x_copy={a: burst[a] / (2 * min(copies)) for a in burst},
         host_over_overlap=(t_labels + t_ref) / burst["reference"])
    ch.close()


def sampled(repeats):
    w, ch = make("c2")
    ch.enable_series(50 * 2 * repeats + 200)
    ch.run(1000)
    ch.set_reference()
    ch.run_sampled(100, 50, overlap=True)  # warm both loops
    plain, measured = [], []
    for _ in range(repeats):
        for out, flag in ((plain, False), (measured, True)):
            t0 = time.perf_counter()
            ch.run_sampled(100, 50, overlap=flag)
            out.append((time.perf_counter() - t0) * 1e3)
    emit(what="sampled", shape="c2", chains=ch.n_chains, loop="50 x (run_async(100), record)",
         plain_ms=plain, with_overlap_ms=measured, plain_spread_ms=max(plain) - min(plain),
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
