#!/usr/bin/env python3
"""Cost of resampling plans across chains (Chains.resample / Chains.clone) at the bench shapes,
one JSON line per shape (raw lines are kept under profiles/resample/).

  shape c3 / c4   after --steps steps: 5 x (resample; sync) under a host clock that ends in the
                  synchronise (so the figure holds the launches' latency as well), 5 resamples
                  enqueued back to back over one synchronise, and the split: the gather alone is
                  clone(last_sources()), the same copies again, so weights-and-scans = resample -
                  gather; clone with 10% / 50% / 90% of the chains replaced (5 x each); the floor,
                  a device-to-device copy of as many label regions (n_chains x label bytes x the
                  fraction replaced; a record also holds its group sums, a few hundred bytes)
                  under HIP events; and the host route {labels(), stats(), numpy gather,
                  fw_chains_write of both} on --host-chains chains, scaled to all of them

    python scripts/resample_bench.py [--only c3|c4] [--steps N] [--chains C]
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

import resample_ref  # noqa: E402
from flipcomplexityempirical_amd import _lib  # noqa: E402
from flipcomplexityempirical_amd._lib import ptr  # noqa: E402
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


def replace_map(C, fraction, rng):
    """A map that replaces ``fraction`` of the chains by clones of the others."""
    src = np.arange(C, dtype=np.int32)
    gone = rng.choice(C, int(round(C * fraction)), replace=False)
    kept = np.setdiff1d(np.arange(C), gone)
    src[gone] = rng.choice(kept, len(gone))
    return src


def d2d_ms(nbytes):
    import torch
    src = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def host_route_ms(name, hc, steps):
    w, ch = make(name, hc)
    ch.run(steps)
    src = replace_map(hc, 0.5, np.random.default_rng(1))
    L = _lib.load()
    t0 = time.perf_counter()
    lab, st, _, _, _ = resample_ref.gather(src, ch.labels(), ch.stats())
    for what, a in ((_lib.READ_LABELS, lab), (_lib.READ_STATS, st)):
        a = np.ascontiguousarray(a)
        _lib.check(L.fw_chains_write(ch._h, what, ptr(a), a.nbytes))
    ms = (time.perf_counter() - t0) * 1e3
    ch.close()
    return ms


def shape(name, steps, chains, host_chains):
    w, ch = make(name, chains)
    C = ch.n_chains
    ch.run(steps)
    b0, b1 = w.base, w.base * 1.1
    ch.resample(b0, b1)
    ch.sync()  # warm: code objects loaded, buffers allocated
    single = timed(ch, lambda: ch.resample(b0, b1))
    info = ch.resample_info()
    t0 = time.perf_counter()
    for _ in range(5):
        ch.resample(b0, b1)
    ch.sync()
    burst = (time.perf_counter() - t0) * 1e3 / 5
    last = ch.last_sources()
    gather = timed(ch, lambda: ch.clone(last))
    bits = ch.overlap_info()["label_bits"]
    lab_bytes = (w.graph.n * bits + 31) // 32 * 4
    rng = np.random.default_rng(0)
    clones, floors = {}, {}
    for frac in (0.1, 0.5, 0.9):
        m = replace_map(C, frac, rng)
        ch.clone(m)
        ch.sync()
        clones[str(frac)] = timed(ch, lambda m=m: ch.clone(m))
        floors[str(frac)] = d2d_ms(int(round(C * frac)) * lab_bytes)
    hc = min(host_chains, C)
    host = host_route_ms(name, hc, min(steps, 1000)) * C / hc
    emit(what="resample", shape=name, chains=C, nodes=w.graph.n, k=w.k, label_bits=bits, steps=steps,
         bases=[b0, b1], resample_sync_ms=single, resample_burst_ms=burst,
         gather_of_last_map_ms=gather, map_ms=min(single) - min(gather),
         replaced_by_last_map=int((last != np.arange(C)).sum()),
         survivors=info["survivors"], max_offspring=info["max_offspring"],
         clone_ms=clones, label_bytes_per_chain=lab_bytes, d2d_copy_ms=floors,
         host_route_ms_scaled=host, host_route_chains=hc,
         host_over_resample=host / min(single))
    ch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["c3", "c4"])
    ap.add_argument("--steps", type=int, default=25000)
    ap.add_argument("--chains", type=int, default=None)
    ap.add_argument("--host-chains", type=int, default=4096)
    a = ap.parse_args()
    for name in ("c3", "c4"):
        if a.only in (None, name):
            shape(name, a.steps, a.chains, a.host_chains)
