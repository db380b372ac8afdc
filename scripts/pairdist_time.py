#!/usr/bin/env python3
"""Cost of the pairwise plan distances (Chains.pair_distances) at the bench shapes, one JSON
line per shape (raw lines are kept under profiles/pairdist/).

  c3   100x100, k = 4, 2-bit labels: symmetric m = 1,024, 4,096 and 16,384; rectangular
       65,536 x 64
  c4   9,000 nodes, k = 18, 5-bit labels: symmetric m = 4,096

Per shape, after --steps steps: 5 warm-up calls, then 20 calls enqueued back to back over one
synchronise under the host clock (the handle's stream is the library's own, so no event of this
process can be recorded on it; both kernels of a measurement are inside the figure), and the
median of 20 x (call; sync).  The host route is labels() plus tests/pairdist_ref.py on
--host-chains members, scaled by the number of pairs; its matrix is compared with the device's
on those members.  The issue bound: --valu VALU instructions per 32-node pair-group of the
inner loop (count them in the ISA of the build) times the pair-groups, over CUs x 4 SIMDs x one
wave instruction per 4 clocks at --mhz.

    python scripts/pairdist_time.py [--only c3|c4] [--steps N] [--host-chains H]
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

import pairdist_ref  # noqa: E402
from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds  # noqa: E402
from flipcomplexityempirical_amd.workloads import workload  # noqa: E402

SHAPES = {"c3": [("sym", 1024, None), ("sym", 4096, None), ("sym", 16384, None),
                 ("rect", 65536, 64)],
          "c4": [("sym", 4096, None)]}


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


def shape(name, steps, host_chains, valu, mhz, cus):
    w = workload(name)
    need = max(m for _, m, _ in SHAPES[name])
    ch = Chains(DeviceGraph(w.graph), max(need, 1), w.k, w.init, proposal=w.proposal,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent), base=w.base, seed=0)
    ch.run(steps)
    t0 = time.perf_counter()
    labels = ch.labels()
    labels_ms = (time.perf_counter() - t0) * 1e3
    n, groups = w.graph.n, (w.graph.n + 31) // 32
    for kind, ma, mb in SHAPES[name]:
        a = np.arange(ma, dtype=np.int32)
        b = None if kind == "sym" else np.arange(mb, dtype=np.int32) * (ma // mb)
        out = {"what": "pairdist", "shape": name, "kind": kind, "ma": ma, "mb": mb or ma,
               "chains": ch.n_chains, "nodes": n, "k": w.k, "steps": steps}
        out["sync_ms"], out["burst_ms"] = timed(ch, lambda: ch.pair_distances(a, b))
        info = ch.pair_distance_info()
        out.update(label_bits=info["label_bits"], tile=info["tile"], chunk=info["chunk"])
        # pairs the first kernel computes: the blocks on or above the diagonal, whole tiles
        t = info["tile"]
        nb_a, nb_b = -(-ma // t), -(-(mb or ma) // t)
        blocks = nb_a * (nb_a + 1) // 2 if kind == "sym" else nb_a * nb_b
        out["pair_groups"] = blocks * t * t * groups
        per = valu or 2 * info["label_bits"]  # lb XOR + (lb - 1) OR + 1 count, without v_or3
        out["valu_per_pair_group"] = per
        out["issue_bound_ms"] = out["pair_groups"] * per / 64 / (cus * 4 * mhz * 1e6 / 4) * 1e3
        out["burst_over_bound"] = out["burst_ms"] / out["issue_bound_ms"]
        # the host route on a subset, scaled by the pairs, and the device against it
        ha = a[:min(host_chains, ma)]
        hb = None if b is None else b[:min(host_chains, len(b))]
        t0 = time.perf_counter()
        want = pairdist_ref.matrix(labels, ha, hb)
        host_ms = (time.perf_counter() - t0) * 1e3
        out["host_ref_members"] = [len(ha), len(ha) if hb is None else len(hb)]
        out["host_labels_ms"] = labels_ms
        out["host_ref_ms_scaled"] = host_ms * (ma * (mb or ma)) / want.size
        out["host_over_device"] = (labels_ms + out["host_ref_ms_scaled"]) / out["burst_ms"]
        ch.pair_distances(ha, hb)
        out["equal_to_host"] = bool(np.array_equal(ch.distance_matrix(), want))
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)
    ch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c3", "c4"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-chains", type=int, default=512)
    ap.add_argument("--valu", type=int, default=0, help="VALU instructions per pair-group (ISA)")
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--cus", type=int, default=256)
    a = ap.parse_args()
    for name in ("c3", "c4"):
        if a.only in (None, name):
            shape(name, a.steps, a.host_chains, a.valu, a.mhz, a.cus)
