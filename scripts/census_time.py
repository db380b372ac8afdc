#!/usr/bin/env python3
"""Cost of an ensemble census (Chains.census) at the bench shapes, one JSON line per shape
(raw lines are kept under profiles/census/).

  shape c3 / c4   after --steps steps, with all three parts and with nodes only: 5 warm-up calls,
                  then 20 x (census; sync) under a host clock that ends in the synchronise (median)
                  and 20 calls enqueued back to back over one synchronise (the handle's stream is
                  the library's own, so no event of this process can be recorded on it; the burst
                  hides the launch latency the single calls include).  On the same handle in the
                  same process, set_reference() with no argument timed the same way: a
                  device-to-device copy of the same label words.  And the host route: labels()
                  plus tests/census_ref.py over --host-chains chains, scaled to all of them, its
                  counts compared with the device's.

    python scripts/census_time.py [--only c3|c4] [--steps N] [--chains C]
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

import census_ref  # noqa: E402
from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds  # noqa: E402
from flipcomplexityempirical_amd.workloads import workload  # noqa: E402


def timed(ch, call, warm=5, n=20):
    """(median ms of n x (call; sync), ms per call of n calls over one sync)"""
    for _ in range(warm):
        call()
    ch.sync()
    single = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ch.sync()
        single.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    ch.sync()
    return float(np.median(single)), (time.perf_counter() - t0) * 1e3 / n


def shape(name, steps, chains, host_chains):
    w = workload(name)
    ch = Chains(DeviceGraph(w.graph), chains or w.chains, w.k, w.init, proposal=w.proposal,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent), base=w.base, seed=0)
    ch.run(steps)
    out = {"what": "census", "shape": name, "chains": ch.n_chains, "nodes": w.graph.n,
           "edges": w.graph.n_edges, "k": w.k, "steps": steps}
    ch.enable_census(True, False, False)
    out["nodes_only_sync_ms"], out["nodes_only_burst_ms"] = timed(ch, ch.census)
    ch.enable_census()
    out["label_bits"] = ch.census_info()["label_bits"]
    out["census_sync_ms"], out["census_burst_ms"] = timed(ch, ch.census)
    out["snapshot_sync_ms"], out["snapshot_burst_ms"] = timed(ch, ch.set_reference)
    out["label_word_bytes"] = ch.n_chains * ((w.graph.n * out["label_bits"] + 31) // 32) * 4
    out["ratio_to_snapshot"] = out["census_burst_ms"] / out["snapshot_burst_ms"]
    # the host route, and the device's counts of one census against it
    ch.census_reset()
    ch.census()
    t0 = time.perf_counter()
    labels = ch.labels()
    out["host_labels_ms"] = (time.perf_counter() - t0) * 1e3
    hc = min(host_chains, ch.n_chains)
    t0 = time.perf_counter()
    ref = None
    for c in range(0, hc, 256):
        ref = census_ref.add(ref, census_ref.census(w.graph, labels[c:c + 256], w.k))
    out["host_ref_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * ch.n_chains / hc
    out["host_ref_chains"] = hc
    out["host_over_census"] = (out["host_labels_ms"] + out["host_ref_ms_scaled"]) / out["census_burst_ms"]
    if hc == ch.n_chains:
        got = {"cnt": ch.census_counts(), "occ": ch.node_occupancy(),
               "ecut": ch.edge_cut_counts(), "bnd": ch.boundary_counts()}
        out["equal_to_host"] = all(np.array_equal(got[key], ref[key]) for key in ref)
    else:  # the part of the sums no subset can check is the total
        out["occupancy_total_ok"] = bool(
            (ch.node_occupancy().sum(axis=2) == ch.census_counts()[:, None]).all())
    out["build"] = _lib.build_info()
    print(json.dumps(out), flush=True)
    ch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c3", "c4"])
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--host-chains", type=int, default=1024)
    a = ap.parse_args()
    for name in ("c3", "c4"):
        if a.only in (None, name):
            shape(name, a.steps, a.chains, a.host_chains)
