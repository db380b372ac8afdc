"""Philox coordinates past 32 bits, bit for bit against the oracle.

include/flipwalk.h documents the proposal draw's counter as (lo32(attempt), hi32(attempt),
lo32(chain), hi32(chain)) under key = the 64-bit seed; the kernels keep 32-bit per-launch
attempt counters that fold into 64-bit totals.  Every other GPU test keeps chain ids near
1,000, seeds small and attempt counters starting at 0, so no high word is ever non-zero and no
carry into one is ever taken.  Here chain ids straddle 2^32 inside one handle (and one wave) or
sit past 2^40, the seed uses its high word (or has a zero low word), and the attempt counters
are moved next to 2^32 (and 2^33) through a checkpoint, so that a launch, a counter fold and a
launch split each carry into the high word.  Those crossings run without sampled waits, so the
lean kernels (the grid kernel with one and with four rows per chain, the one-chain-per-wave
and the padded-row kernels) take the carry; two of them are repeated with sampled waits on,
which selects the FULL instantiations and whose counter ORs 2^31 into the same word.  The
exchange and the resample draws are taken past 2^32 too.  The grid cases read the rows per chain
back from the library's FLIPWALK_VERBOSE plan line.
"""
import numpy as np
import pytest

import resample_ref
from cases import cases
from flipcomplexityempirical_amd import population
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, wait_prob_table
from ladder_ref import tempered_ref
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases()}
KNOBS = ("FLIPWALK_NO_GRID16", "FLIPWALK_SPEC", "FLIPWALK_FOLD_AT", "FLIPWALK_LAUNCH_STEPS",
         "FLIPWALK_W2", "FLIPWALK_CSR_LB", "FLIPWALK_GRID_CAP", "FLIPWALK_SLICES")
# the grid kernel (and with four speculative rows), the one-chain-per-wave kernel on the same
# grid, the padded-row kernel on the sec11 graph and on the Kansas tracts
KERNELS = [("grid20_k4_mu", {"FLIPWALK_SPEC": "1"}), ("grid20_k4_mu", {"FLIPWALK_SPEC": "4"}),
           ("grid20_k4_mu", {"FLIPWALK_NO_GRID16": "1"}), ("sec11_a2_k2", {}), ("tract_k4", {})]
KERNEL_IDS = ["grid", "grid-spec4", "wave64", "sec11", "tract"]
N_CHAINS = 13
BIG_SEED = 0x9E3779B97F4A7C15


def set_knobs(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("FLIPWALK_VERBOSE", "1")
    for key, value in env.items():
        monkeypatch.setenv(key, value)


def assert_plan(env, err):
    """The kernel the case means ran: the grid kernel with the rows per chain asked for, or
    the one-chain-per-wave kernel."""
    grid = [ln for ln in err.splitlines() if ln.startswith("flipwalk: grid kernel")]
    chain = [ln for ln in err.splitlines() if ln.startswith("flipwalk: chain kernel")]
    if "FLIPWALK_SPEC" in env:
        assert grid and not chain, err
        for ln in grid:
            assert f"{env['FLIPWALK_SPEC']} row(s) per chain" in ln, ln
    else:
        assert chain and not grid, err


def assert_stats_equal(gpu, orc):
    for f in orc.dtype.names:
        a, b = gpu[f], orc[f]
        if f == "sum_invb":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (f, a, b)


def make(case, dg, seed, id0):
    return Chains(dg, N_CHAINS, case.k, case.init, proposal=case.mode, pop_bounds=case.bounds,
                  base=case.base, seed=seed, chain_id0=id0)


COORDS = [("ids-straddle-2^32", 99, 2**32 - 6), ("ids-past-2^40", 99, 2**40 + 3),
          ("seed-high-word", BIG_SEED, 3), ("seed-low-word-zero", 2**32, 3),
          ("all-high-words", BIG_SEED, 2**40 + 2**32 - 6)]


@pytest.mark.parametrize("what,seed,id0", COORDS, ids=[c[0] for c in COORDS])
@pytest.mark.parametrize("name,env", KERNELS, ids=KERNEL_IDS)
def test_chain_ids_and_seeds_past_32_bits(gpu_lib, name, env, what, seed, id0, monkeypatch,
                                          capfd):
    """13 chains, launches of 500 and 700 steps: plans, every counter, sum_invb bitwise, the
    populations and both histograms equal the oracle's."""
    set_knobs(monkeypatch, env)
    case = CASES[name]
    g, (lo, hi) = case.graph, case.bounds
    capfd.readouterr()
    dg = DeviceGraph(g)
    ch = make(case, dg, seed, id0)
    for s in (500, 700):
        ch.run(s)
    assert_plan(env, capfd.readouterr().err)
    hc, hb = np.zeros(g.n_edges + 1, np.uint64), np.zeros(g.n + 1, np.uint64)
    labels, stats, pops = ch.labels(), ch.stats(), ch.pops()
    for i in range(N_CHAINS):
        lab, st = case.init, O.new_stats(1)
        for s in (500, 700):
            lab, st, p, _ = O.run_chain(g, lab, case.k, case.mode, lo, hi, case.thr, seed, id0 + i,
                                        s, stats=st, hist_cut=hc, hist_b=hb)
        assert np.array_equal(labels[i], lab), i
        assert_stats_equal(stats[i:i + 1], st)
        assert np.array_equal(pops[i], p), i
    assert np.array_equal(ch.hist_cut(), hc) and np.array_equal(ch.hist_b(), hb)
    assert (stats["steps"] == 1200).all()


FOLD, SPLIT = {"FLIPWALK_FOLD_AT": "64"}, {"FLIPWALK_LAUNCH_STEPS": "97"}
# (id, where the attempt counters are put, knobs, sampled waits)
CROSSINGS = [("cross-2^32", 2**32 - 300, {}, False), ("cross-2^32-fold", 2**32 - 300, FOLD, False),
             ("cross-2^32-split", 2**32 - 300, SPLIT, False),
             ("cross-2^33", 2**33 - 300, {}, False), ("cross-2^33-fold", 2**33 - 300, FOLD, False),
             ("cross-2^33-split", 2**33 - 300, SPLIT, False),
             ("cross-2^32-waits", 2**32 - 300, {}, True), ("cross-2^33-waits", 2**33 - 300, FOLD, True)]


@pytest.mark.parametrize("what,target,extra,with_waits", CROSSINGS, ids=[c[0] for c in CROSSINGS])
@pytest.mark.parametrize("name,env", KERNELS, ids=KERNEL_IDS)
def test_attempt_counter_crosses_a_word_boundary(gpu_lib, name, env, what, target, extra,
                                                 with_waits, monkeypatch, capfd):
    """50 steps, a checkpoint whose attempt counters are moved to ``target`` (the same offset
    added to pop_fail, so the record stays consistent), restored into a new handle that runs
    400 and 300 steps: every chain's attempt counter carries into its high word during the
    first launch (at 2^33 - 300 the high word is non-zero before it).  The oracle is fed the
    same edited record.  Without sampled waits the lean kernels run (with four rows per chain
    in the grid-spec4 cases); with them the FULL ones, and the wait draws, whose counter ORs
    2^31 into hi32(attempt), are compared too."""
    set_knobs(monkeypatch, {**env, **extra})
    case = CASES[name]
    g, (lo, hi) = case.graph, case.bounds
    seed, id0 = BIG_SEED, 2**32 - 6
    capfd.readouterr()
    dg = DeviceGraph(g)
    a = make(case, dg, seed, id0)
    if with_waits:
        a.enable_sampled_waits()
    a.run(50)
    ck = a.checkpoint()
    st = ck["stats"]
    assert (st["attempts"] < 2**31).all()
    offset = np.uint64(target) - st["attempts"]
    st["attempts"] += offset
    st["pop_fail"] += offset
    assert (st["attempts"] == target).all()
    b = make(case, dg, seed, id0)
    b.restore(ck)
    for s in (400, 300):
        b.run(s)
    assert_plan(env, capfd.readouterr().err)
    assert b.waits_on == with_waits
    labels, stats, pops = b.labels(), b.stats(), b.pops()
    waits = b.waits() if with_waits else None
    hc, hb = np.zeros(g.n_edges + 1, np.uint64), np.zeros(g.n + 1, np.uint64)
    pt = wait_prob_table(g.n, case.k)
    for i in range(N_CHAINS):
        w = O.Waits(pt) if with_waits else None
        lab, ost, _, _ = O.run_chain(g, case.init, case.k, case.mode, lo, hi, case.thr, seed,
                                     id0 + i, 50, hist_cut=hc, hist_b=hb, waits=w)
        assert np.array_equal(ck["labels"][i], lab), i
        ost["attempts"] += offset[i]
        ost["pop_fail"] += offset[i]
        assert_stats_equal(st[i:i + 1], ost)
        for s in (400, 300):
            lab, ost, p, _ = O.run_chain(g, lab, case.k, case.mode, lo, hi, case.thr, seed,
                                         id0 + i, s, stats=ost, hist_cut=hc, hist_b=hb, waits=w)
        assert np.array_equal(labels[i], lab), i
        assert_stats_equal(stats[i:i + 1], ost)
        assert np.array_equal(pops[i], p), i
        if with_waits:
            assert np.array([w.sum, w.cur]).tobytes() == waits[i].tobytes(), (i, w.sum, waits[i])
    assert np.array_equal(b.hist_cut(), hc) and np.array_equal(b.hist_b(), hb)
    assert (stats["attempts"] > (target | 0xFFFFFFFF)).all()  # every chain took the carry


# the bases are close enough for the reference to take and to refuse swaps in 8 rounds
@pytest.mark.parametrize("name,path,bases", [("grid12_k4_pairs", "auto", (0.95, 1.05)),
                                             ("grid12_k4_pairs", "wave64", (0.95, 1.05)),
                                             ("hub_k3", "auto", (0.9, 1.1))])
def test_exchange_draws_past_32_bits(gpu_lib, name, path, bases, monkeypatch):
    """Replica exchange with the sets' smallest chain ids on both sides of 2^32 and a seed that
    uses its high word: 8 rounds of 40 steps against ladder_ref.tempered_ref, bit for bit."""
    set_knobs(monkeypatch, {"FLIPWALK_NO_GRID16": "1"} if path == "wave64" else {})
    case = CASES[name]
    n_rungs, n_sets, id0, round0 = 2, 4, 2**32 - 3, 2**32 - 9
    s = np.arange(n_rungs * n_sets, dtype=np.int32) // n_rungs
    r = np.arange(n_rungs * n_sets, dtype=np.int32) % n_rungs
    ref = tempered_ref(case.graph, case.init, case.k, case.mode, case.bounds, bases, s, r,
                       BIG_SEED, id0, 40, 8, round0)
    rs = ref["rung_stats"]
    assert 0 < rs["swap_done"].sum() < rs["swap_tried"].sum()
    dg = DeviceGraph(case.graph)
    ch = Chains(dg, n_rungs * n_sets, case.k, case.init, proposal=case.mode,
                pop_bounds=case.bounds, base=case.base, seed=BIG_SEED, chain_id0=id0)
    ch.set_ladder(bases, s, r)
    ch.run_tempered(40, 8, round0=round0)
    assert np.array_equal(ch.labels(), ref["labels"])
    assert np.array_equal(ch.rungs(), ref["rungs"])
    assert_stats_equal(ch.stats(), ref["stats"])
    got = ch.rung_stats()
    for f in rs.dtype.names:
        a, b = got[f], rs[f]
        if f == "sum_invb":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), f


@pytest.mark.parametrize("id0,round", [(2**32 - 6, 3), (2**40 + 3, 2**31 + 5)])
def test_resample_draw_past_32_bits(gpu_lib, id0, round, monkeypatch):
    """The one Philox block of a resample with chain_id0 past 2^32 (and a round past 2^31):
    weights and the source map against resample_ref."""
    set_knobs(monkeypatch, {})
    case = CASES["grid12_k4_pairs"]
    dg = DeviceGraph(case.graph)
    ch = Chains(dg, 77, case.k, case.init, proposal=case.mode, pop_bounds=case.bounds,
                base=case.base, seed=BIG_SEED, chain_id0=id0)
    ch.run(200)
    cut = ch.stats()["cut"]
    q, sign = population.weight_table(case.base, case.base * 1.3, dg.n_edges)
    ref = resample_ref.resample_map(cut, q, sign, resample_ref.draw_u(BIG_SEED, round, id0))
    ch.resample(case.base, case.base * 1.3, round=round)
    assert np.array_equal(ch.last_weights(), ref["W"])
    assert np.array_equal(ch.last_sources(), ref["src"])
