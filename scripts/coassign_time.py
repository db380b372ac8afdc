#!/usr/bin/env python3
"""Cost of the node co-assignment step (Chains.coassign) at the C3 shape (100x100, k = 4,
65,536 chains, 2-bit labels), one JSON line per list (raw lines are kept under
profiles/coassign/): m = 1,024 evenly spaced nodes, and m = n.

Per list, after --steps steps: 3 warm-up calls, then --calls calls enqueued back to back over one
synchronise under the host clock (the handle's stream is the library's own, so no event of this
process can be recorded on it; both kernels of a measurement are inside the figure).  The split
between the two kernels is taken from a kernel trace of this script, not from here.  Beside it:
the host route, labels() plus tests/coassign_ref.py on --host-chains chains scaled by the chain
count (extrapolated), and the product's pair-words per second (entry pairs of the blocks on or
above the diagonal, whole tiles, times member words) next to fw_pairdist's pair-groups per second
measured in the same run at symmetric m = 16,384, which is the same arithmetic.

    python scripts/coassign_time.py [--steps N] [--calls K] [--host-chains H] [--skip-full]
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

import coassign_ref  # noqa: E402
from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds  # noqa: E402
from flipcomplexityempirical_amd.workloads import workload  # noqa: E402


def burst(ch, call, warm, n):
    for _ in range(warm):
        call()
    ch.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    ch.sync()
    return (time.perf_counter() - t0) * 1e3 / n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-chains", type=int, default=128)
    ap.add_argument("--skip-full", action="store_true", help="leave out m = n")
    a = ap.parse_args()
    w = workload("c3")
    n = w.graph.n
    ch = Chains(DeviceGraph(w.graph), 65536, w.k, w.init, proposal=w.proposal,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent), base=w.base, seed=0)
    ch.run(a.steps)
    t0 = time.perf_counter()
    labels = ch.labels()
    labels_ms = (time.perf_counter() - t0) * 1e3
    # the yardstick: the same arithmetic over nodes instead of members
    members = np.arange(16384, dtype=np.int32)
    pwd_ms = burst(ch, lambda: ch.pair_distances(members), 3, a.calls)
    pinfo = ch.pair_distance_info()
    pblocks = -(-16384 // pinfo["tile"])
    pwd_rate = pblocks * (pblocks + 1) // 2 * pinfo["tile"] ** 2 * ((n + 31) // 32) / (pwd_ms * 1e-3)
    lists = [("spaced", np.arange(1024) * n // 1024)] + ([] if a.skip_full else [("all", None)])
    for name, nodes in lists:
        ch.enable_coassignment(nodes)
        info = ch.coassign_info()
        m = info["m"]
        out = {"what": "coassign", "shape": "c3", "list": name, "m": m, "chains": ch.n_chains,
               "nodes": n, "k": w.k, "steps": a.steps, "calls": a.calls}
        out.update(label_bits=info["label_bits"], tile=info["tile"], chunk=info["chunk"],
                   staged=info["staged"])
        out["burst_ms"] = burst(ch, ch.coassign, 3, a.calls)
        words, blocks = (ch.n_chains + 31) // 32, -(-m // info["tile"])
        out["pair_words"] = blocks * (blocks + 1) // 2 * info["tile"] ** 2 * words
        out["pair_words_per_s"] = out["pair_words"] / (out["burst_ms"] * 1e-3)
        out["pairdist_m16384_ms"] = pwd_ms
        out["pairdist_pair_groups_per_s"] = pwd_rate
        out["rate_over_pairdist"] = out["pair_words_per_s"] / pwd_rate
        if name == "spaced":  # cheap to read back: the invariants of the accumulated matrix
            t, cnt = ch.coassignment(), ch.coassign_counts()
            out["symmetric_and_diagonal_cnt"] = bool(
                np.array_equal(t, t.transpose(0, 2, 1)) and (np.diagonal(t[0]) == cnt[0]).all())
            want = coassign_ref.coassign(labels, w.k, nodes)
            out["equal_to_host"] = bool(np.array_equal(
                t[0], want["together"][0] * np.uint64(info["n_measured"] + 3 + a.calls)))
        h = min(a.host_chains, ch.n_chains)
        t0 = time.perf_counter()
        coassign_ref.coassign(labels[:h], w.k, nodes)
        host_ms = (time.perf_counter() - t0) * 1e3
        out["host_ref_chains"] = h
        out["host_labels_ms"] = labels_ms
        out["host_ref_ms_extrapolated"] = host_ms * ch.n_chains / h
        out["host_over_device"] = (labels_ms + out["host_ref_ms_extrapolated"]) / out["burst_ms"]
        out["build"] = _lib.build_info()
        print(json.dumps(out), flush=True)
    ch.close()
