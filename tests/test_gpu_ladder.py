"""Replica exchange across a base ladder on the GPU (fw_chains_set_ladder /
fw_chains_exchange_async) against the CPU restatement in ladder_ref.py, bit for bit, plus
the handle's bookkeeping around it: stream ordering, checkpoint / resume, refusals, the
re-snapshot rules, and the law each rung keeps."""
import functools

import numpy as np
import pytest

from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import grid_graph, stripe_seed
from ladder_ref import tempered_ref

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
SEED, ID0, ROUND0, ROUNDS, STEPS = 2024, 17, 5, 12, 50
# case -> (n_rungs, n_sets)
SHAPES = {"grid12_k4_pairs": (4, 3), "grid7x9_k3_cut": (3, 2), "hub_k3": (2, 3),
          "grid10_k2_bi": (64, 1)}
# case -> (lowest, highest base).  Over [0.5, 2] the two short ladders' neighbouring rungs are
# so far apart that the reference accepts no swap in 12 rounds; closer bases give both outcomes
BASE_RANGE = {"grid7x9_k3_cut": (0.7, 1.4), "hub_k3": (0.9, 1.1)}
BIT_EXACT = [("grid12_k4_pairs", "auto"), ("grid12_k4_pairs", "wave64"),
             ("grid7x9_k3_cut", "auto"), ("hub_k3", "auto"), ("grid10_k2_bi", "auto")]


def scrambled_layout(n_rungs, n_sets):
    c = np.arange(n_rungs * n_sets)
    s = c % n_sets
    return s.astype(np.int32), ((c // n_sets + s) % n_rungs).astype(np.int32)


def ladder_bases(n_rungs, name=None):
    return np.geomspace(*BASE_RANGE.get(name, (0.5, 2.0)), n_rungs)


@functools.lru_cache(maxsize=None)
def reference(name):
    case = CASES[name]
    n_rungs, n_sets = SHAPES[name]
    s, r = scrambled_layout(n_rungs, n_sets)
    return tempered_ref(case.graph, case.init, case.k, case.mode, case.bounds,
                        ladder_bases(n_rungs, name), s, r, SEED, ID0, STEPS, ROUNDS, ROUND0)


def make(name, seed=SEED):
    case = CASES[name]
    n_rungs, n_sets = SHAPES[name]
    dg = DeviceGraph(case.graph)
    ch = Chains(dg, n_rungs * n_sets, case.k, case.init, proposal=case.mode,
                pop_bounds=case.bounds, base=case.base, seed=seed, chain_id0=ID0)
    ch.set_ladder(ladder_bases(n_rungs, name), *scrambled_layout(n_rungs, n_sets))
    return ch


def snapshot(ch):
    return {"labels": ch.labels(), "stats": ch.stats(), "pops": ch.pops(),
            "hist_cut": ch.hist_cut(), "hist_b": ch.hist_b(), "rungs": ch.rungs(),
            "rung_stats": ch.rung_stats()}


def assert_same(got, want):
    for key in ("labels", "pops", "hist_cut", "hist_b", "rungs"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("stats", "rung_stats"):
        for f in want[key].dtype.names:
            a, b = got[key][f], want[key][f]
            if f == "sum_invb":  # bitwise
                a, b = a.view(np.uint64), b.view(np.uint64)
            assert np.array_equal(a, b), (key, f, a, b)


@pytest.mark.parametrize("name,kernel_path", BIT_EXACT, ids=[f"{p}-{n}" for n, p in BIT_EXACT])
def test_tempered_bit_exact(gpu_lib, name, kernel_path, monkeypatch):
    """12 rounds x 50 steps from round 5 (odd parity first), scrambled placement, global chain
    ids from 17: plans, every stats field, populations, both histograms, the rungs and the
    rung stats equal the reference's; sum_invb bitwise in both records."""
    if kernel_path == "wave64":
        monkeypatch.setenv("FLIPWALK_NO_GRID16", "1")
    else:
        monkeypatch.delenv("FLIPWALK_NO_GRID16", raising=False)
    ref = reference(name)
    rs = ref["rung_stats"]
    done, tried = int(rs["swap_done"].sum()), int(rs["swap_tried"].sum())
    print(f"{name}: reference swaps {done} of {tried}")
    # the case must exercise both outcomes of the rule
    assert done >= 1 and tried - done >= 1
    ch = make(name)
    ch.run_tempered(STEPS, ROUNDS, round0=ROUND0)
    assert ch.ladder_round == ROUND0 + ROUNDS
    assert_same(snapshot(ch), ref)
    n_rungs, n_sets = SHAPES[name]
    assert ch.rung_stats().shape == (n_sets, n_rungs)
    # every set still holds one chain per rung
    s, _ = scrambled_layout(n_rungs, n_sets)
    for i in range(n_sets):
        assert sorted(ch.rungs()[s == i].tolist()) == list(range(n_rungs))


def test_run_tempered_equals_stepwise(gpu_lib):
    """The back-to-back enqueue of run_tempered orders runs and exchanges on the stream as
    twelve blocking run / exchange calls with reads in between do."""
    name = "grid12_k4_pairs"
    a = make(name)
    a.run_tempered(STEPS, ROUNDS, round0=ROUND0)
    b = make(name)
    for i in range(ROUNDS):
        b.run(STEPS)
        b.stats()
        b.exchange(ROUND0 + i)
        b.rungs()
    assert_same(snapshot(a), snapshot(b))
    assert_same(snapshot(a), reference(name))


def test_ladder_checkpoint_resume(gpu_lib, tmp_path):
    name = "grid12_k4_pairs"
    whole = make(name)
    whole.ladder_round = ROUND0
    whole.run_tempered(STEPS, ROUNDS)
    first = make(name)
    first.ladder_round = ROUND0
    first.run_tempered(STEPS, ROUNDS // 2)
    path = str(tmp_path / "ladder.npz")
    first.save_checkpoint(path)
    case = CASES[name]
    resumed = Chains.from_checkpoint(DeviceGraph(case.graph), path, case.k)
    assert resumed.ladder_round == ROUND0 + ROUNDS // 2
    assert np.array_equal(resumed.rungs(), first.rungs())
    assert_same(snapshot(resumed), snapshot(first))
    resumed.run_tempered(STEPS, ROUNDS - ROUNDS // 2)
    assert resumed.ladder_round == whole.ladder_round == ROUND0 + ROUNDS
    assert_same(snapshot(resumed), snapshot(whole))
    assert_same(snapshot(resumed), reference(name))


def test_ladder_refusals(gpu_lib):
    case = CASES["grid12_k4_pairs"]
    n_rungs, n_sets = 4, 3
    bases = ladder_bases(n_rungs)

    def fresh():
        return Chains(DeviceGraph(case.graph), n_rungs * n_sets, case.k, case.init,
                      proposal=case.mode, pop_bounds=case.bounds, base=case.base, seed=SEED)

    def still_runs(ch, steps_before):
        ch.run(20)
        st = ch.stats()
        assert (st["steps"] == steps_before + 20).all() and not st["stuck"].any()

    def refused(code, fn, *args):
        with pytest.raises(_lib.FlipwalkError) as e:
            fn(*args)
        assert e.value.code == code, e.value

    ch = fresh()  # the rule or a schedule set first: no ladder
    ch.set_accept("bratio")
    refused(_lib.FW_EUNSUPPORTED, ch.set_ladder, bases)
    still_runs(ch, 0)
    ch.set_accept("cut")
    rows = np.stack([case.thr, case.thr])
    ch.set_schedule(rows, 0)
    refused(_lib.FW_EUNSUPPORTED, ch.set_ladder, bases)
    still_runs(ch, 20)
    ch.set_schedule(None)
    refused(_lib.FW_EINVAL, ch.exchange, 0)  # no ladder yet
    with pytest.raises(ValueError):
        ch.run_tempered(10, 1)
    still_runs(ch, 40)
    # a bad layout, on the Python side and (past it) on the C side
    s, r = scrambled_layout(n_rungs, n_sets)
    bad = r.copy()
    bad[0] = bad[n_sets]
    with pytest.raises(ValueError):
        ch.set_ladder(bases, s, bad)
    L = _lib.load()
    rows4 = np.ascontiguousarray(np.stack([case.thr] * n_rungs))
    logb = np.log(bases)
    assert L.fw_chains_set_ladder(ch._h, _lib.ptr(rows4), _lib.ptr(logb), n_rungs, _lib.ptr(s),
                                  _lib.ptr(bad)) == _lib.FW_EINVAL
    assert L.fw_chains_set_ladder(ch._h, _lib.ptr(rows4), _lib.ptr(logb), 5, _lib.ptr(s),
                                  _lib.ptr(r)) == _lib.FW_EINVAL
    refused(_lib.FW_EINVAL, ch.exchange, 0)  # the refused calls left no ladder behind
    still_runs(ch, 60)
    # with a ladder: the other rules and a schedule are refused, the ladder stays
    ch.set_ladder(bases, s, r)
    refused(_lib.FW_EUNSUPPORTED, ch.set_accept, "bratio")
    refused(_lib.FW_EUNSUPPORTED, ch.set_accept, "boundary", np.ones(case.graph.n, np.uint8))
    refused(_lib.FW_EUNSUPPORTED, ch.set_schedule, rows, 0)
    refused(_lib.FW_EINVAL, ch.exchange, -1)
    refused(_lib.FW_EINVAL, ch.exchange, 2 ** 32)
    ch.set_accept("cut")
    ch.set_schedule(None)
    assert ch.accept_rule == _lib.ACCEPT_CUT
    still_runs(ch, 80)
    ch.exchange(0)
    assert sorted(ch.rungs()[s == 0].tolist()) == list(range(n_rungs))
    assert int(ch.rung_stats()["steps"].sum()) == 20 * n_rungs * n_sets


def test_reset_and_stats_write_resnapshot(gpu_lib):
    name = "grid12_k4_pairs"
    n_rungs, n_sets = SHAPES[name]
    ch = make(name)
    ch.run_tempered(STEPS, 3, round0=0)
    assert int(ch.rung_stats()["yields"].sum()) == (3 * STEPS + 1) * n_rungs * n_sets
    ch.reset_observables()
    rs = ch.rung_stats()
    assert all(not rs[f].any() for f in rs.dtype.names)
    ch.run(STEPS)
    before, rungs = ch.stats(), ch.rungs()
    s, _ = scrambled_layout(n_rungs, n_sets)
    ch.exchange(3)
    rs = ch.rung_stats()
    # the round's deltas are the round's own sums: the stats were zeroed with the snapshot
    for f in ("yields", "sum_cut", "sum_bnodes"):
        assert np.array_equal(rs[f][s, rungs], before[f]), f
    assert np.array_equal(rs["sum_invb"][s, rungs].view(np.uint64),
                          before["sum_invb"].view(np.uint64))
    assert (rs["yields"] == STEPS).all() and (rs["steps"] == STEPS).all()
    # a stats write re-snapshots: nothing of the written records reaches the rung stats
    st = ch.stats()
    st["yields"] += 1000
    st["sum_cut"] += 12345
    _lib.check(_lib.load().fw_chains_write(ch._h, _lib.READ_STATS, _lib.ptr(st), st.nbytes))
    ch.exchange(4)
    rs2 = ch.rung_stats()
    for f in ("yields", "steps", "accepts", "sum_cut", "sum_bnodes"):
        assert np.array_equal(rs2[f], rs[f]), f
    assert np.array_equal(rs2["sum_invb"].view(np.uint64), rs["sum_invb"].view(np.uint64))
    # set_ladder again restarts the rung stats
    ch.set_ladder(ladder_bases(n_rungs), s, ch.rungs())
    assert not ch.rung_stats()["swap_tried"].any() and ch.ladder_round == 0


def rung_means(sum_cut, yields):
    """Per-rung mean cut (sum over sets of sum_cut / sum over sets of yields) and its standard
    error across the independent sets; arrays [n_sets, n_rungs]."""
    per_set = sum_cut.astype(np.float64) / yields.astype(np.float64)
    mean = sum_cut.sum(0, dtype=np.float64) / yields.sum(0, dtype=np.float64)
    return mean, per_set.std(0, ddof=1) / np.sqrt(per_set.shape[0])


LAW = dict(w=8, h=8, k=2, percent=0.5, n_rungs=4, n_sets=128, burn=2000, rounds=40, steps=100)


def test_tempering_keeps_rung_law(gpu_lib):
    """Exchanges leave each rung's stationary law alone: after a burn-in, the per-rung mean
    cut of 128 tempered sets equals that of untempered chains at the same bases (existing
    code, another seed) within 4 combined standard errors taken across sets (sets are
    independent; 4 SE leaves room for the four simultaneous comparisons)."""
    p = LAW
    g = grid_graph(p["w"], p["h"])
    init = stripe_seed(p["w"], p["h"])
    n_rungs, n_sets = p["n_rungs"], p["n_sets"]
    bases = ladder_bases(n_rungs)
    bounds = population_bounds(g.total_pop, p["k"], p["percent"])
    C = n_rungs * n_sets
    dg = DeviceGraph(g)
    t = Chains(dg, C, p["k"], init, proposal="bi", pop_bounds=bounds, base=1.0, seed=1)
    t.set_ladder(bases)
    t.run(p["burn"])
    t.reset_observables()
    t.run_tempered(p["steps"], p["rounds"], round0=0)
    rs = t.rung_stats()
    assert (rs["yields"] == p["steps"] * p["rounds"]).all()
    assert int(rs["swap_done"].sum()) > 0
    u = Chains(dg, C, p["k"], init, proposal="bi", pop_bounds=bounds,
               base=np.tile(bases, n_sets), seed=2)
    u.run(p["burn"])
    u.reset_observables()
    u.run(p["steps"] * p["rounds"])
    st = u.stats().reshape(n_sets, n_rungs)
    mt, se_t = rung_means(rs["sum_cut"], rs["yields"])
    mu, se_u = rung_means(st["sum_cut"], st["yields"])
    se = np.sqrt(se_t ** 2 + se_u ** 2)
    print("tempered", mt, "untempered", mu, "4 se", 4 * se)
    assert (np.abs(mt - mu) <= 4 * se).all(), (mt, mu, se)
