"""bench.py's PMC bookkeeping (CPU): a stored profile fills a line's traffic / issue /
occupancy / L2 fields only when it was taken on the same workload, protocol, settings and
build, and its timed launches ran within 10% of the line's kernel time."""
import pytest

import bench


def _ident(**kw):
    d = {"config": "c3", "order": None, "grid": None, "k": 4, "proposal": "pairs",
         "base": "base mu", "percent": 0.05, "seed": 0, "chains": 65536, "chain_id0": 0,
         "inner": 1000, "warmup": 5, "steps": 20, "resumed_steps": 0, "maps": False,
         "flipwalk_env": {}, "build": "src=0123456789abcdef flags=-O3"}
    d.update(kw)
    return d


def test_pmc_key_names_the_protocol():
    assert bench.pmc_key("c3", None, 65536, 1000, 5, 20) == "c3_65536_1000_w5_s20"
    assert bench.pmc_key("c3", None, 8192, 1000, 5, 20, 8192) == "c3_8192_1000_w5_s20_id8192"
    assert bench.pmc_key("c5", None, 8192, 1000, 10, 100, 0, 100000) == "c5_8192_1000_w10_s100_r100000"
    assert bench.pmc_key("c4", "random", 16384, 1000, 5, 20) == "c4r_16384_1000_w5_s20"
    assert bench.pmc_key("c4", "hilbert", 16384, 1000, 5, 20) == "c4_16384_1000_w5_s20"


def test_pmc_mismatch_accepts_only_the_same_run():
    prof = {"source": "profiles/r05/x", "identity": _ident(), "kernel_trace": {"avg_ms": 15.2}}
    assert bench.pmc_mismatch(prof, _ident(), 16.0) is None  # 5% apart
    assert "more than 10%" in bench.pmc_mismatch(prof, _ident(), 17.5)
    why = bench.pmc_mismatch(prof, _ident(build="src=ffffffffffffffff flags=-O3"), 15.2)
    assert why and "build" in why
    assert "flipwalk_env" in bench.pmc_mismatch(prof, _ident(flipwalk_env={"FLIPWALK_SPEC": "2"}), 15.2)
    assert "grid" in bench.pmc_mismatch(prof, _ident(grid=40), 15.2)
    assert "no PMC profile" in bench.pmc_mismatch(None, _ident(), 15.2)
    assert "no identity" in bench.pmc_mismatch({"source": "old"}, _ident(), 15.2)


def test_committed_profiles_match_the_in_tree_library():
    """Every stored profile is named by its own protocol and was taken with the library the
    tree ships, so the driver's lines use it: a kernel change without re-profiling fails
    here (on CPU), not silently as ``pmc.used: false`` in the round's bench line.  The
    driver's protocol (``--steps 20 --warmup 5``, C3, default launch length) must be among
    them."""
    import glob
    import json
    import os
    from flipcomplexityempirical_amd._lib import build_info

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "profiles", "pmc", "*.json")))
    assert files, "no PMC profiles under profiles/pmc"
    build = build_info()
    for f in files:
        prof = json.load(open(f))
        ident = prof["identity"]
        key = bench.pmc_key(ident["config"], ident["order"], ident["chains"], ident["inner"],
                            ident["warmup"], ident["steps"], ident["chain_id0"],
                            ident["resumed_steps"])
        assert os.path.basename(f) == key + ".json", f
        assert ident["build"] == build, f"{f}: profiled build {ident['build']!r}, tree {build!r}"
        assert ident["flipwalk_env"] == {}, f
    keys = {os.path.basename(f)[:-5] for f in files}
    assert bench.pmc_key("c3", None, 65536, 5000, 5, 20) in keys


def test_full_and_dump_outputs_are_options():
    """``--full`` is off by default, and both new options parse beside the driver's."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_chains_hold(tmp_path, gpu_lib):
    """A plain ``bench.py --gpus 1 --steps K --warmup W`` runs nothing but its launches (no
    checker, secondary or CPU legs on the line), times exactly K launches, and
    ``--dump-outputs`` writes float arrays of at most 64 MB that equal, bit for bit, what the
    same chains hold when this process runs them: the same arguments give the same files."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np

    from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
    from flipcomplexityempirical_amd.workloads import workload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "dump")
    n, inner, warm, steps = 600, 100, 1, 3
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", str(warm), "--chains", str(n), "--inner",
                        str(inner), "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["parity_check"] is None
    assert not {"secondary", "cpu_baseline", "cpu_native"} & set(line)
    assert line["hist_yields"] == n * ((warm + steps) * inner + 1)
    files = sorted(os.listdir(out))
    arrs = {f[:-4]: np.load(os.path.join(out, f), allow_pickle=False) for f in files}
    assert all(f.endswith(".npy") for f in files)
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 * 2 ** 20

    w = workload("c3")
    dg = DeviceGraph(w.graph, device=0)
    ch = Chains(dg, n, w.k, w.init, proposal=w.proposal, base=w.base, seed=0,
                pop_bounds=population_bounds(w.graph.total_pop, w.k, w.percent))
    ch.run((warm + steps) * inner)
    st, labels = ch.stats(), ch.labels()
    pick = arrs["label_chains"].astype(np.int64)
    assert len(pick) == min(n, bench.DUMP_LABEL_CHAINS) == len(set(pick.tolist()))
    assert np.array_equal(arrs["labels"], labels[pick].astype(np.float32))
    for f in bench.STAT_FIELDS:
        assert np.array_equal(arrs["stats_" + f], st[f].astype(np.float64)), f
    assert np.array_equal(arrs["pops"], ch.pops().astype(np.float64))
    assert np.array_equal(arrs["hist_cut"], ch.hist_cut().astype(np.float64))
    assert np.array_equal(arrs["hist_b"], ch.hist_b().astype(np.float64))
    ch.close()
    dg.close()
