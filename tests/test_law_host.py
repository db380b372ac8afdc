"""The oracle against the exact law of the chain (law_ref.py: plain Python over networkx, no
oracle code, no Philox).

Bit-exact parity ties the kernels to oracle/flipchain_oracle.c; these tests tie the oracle to
an independent derivation of what a counted step does: proposals uniform over (node, foreign
district) pairs or over cut-edge ends, invalid proposals retried without being counted,
Metropolis acceptance on the tabulated bound, the state re-yielded on rejection, and draws
independent across attempts and chain ids.  20,000 oracle chains (contiguous chain ids, one
seed) per case:

* the plans after t steps against P^t(x0, .): every observed plan inside the exact support, and
  a chi-square goodness of fit with p >= 1e-6 (about 150 deterministic cases: family-wise
  false-alarm chance near 1e-4; seeds are fixed, so a pass stays a pass);
* every counter of ``law_ref.COUNTERS`` as the across-chain mean against its exact expectation,
  |z| <= 5 with the standard error from the across-chain sample variance; yields == t + 1 and
  steps == t exactly;
* the stationary law on 4 x 4, k = 2; the halves of the chain-id range against each other; a
  two-rung replica exchange against the exact joint law;
* five deliberately wrong laws (law_ref ``variant=``), each rejected on the same oracle data.
"""
import functools
import math

import numpy as np
import pytest

import law_cases as LC
import law_ref
from cases import MU
from oracle import oracle as O

N = 20000
SEED = 20241021
P_MIN = LC.P_MIN
GRAPHS = ("g4x4", "g3x5", "g4x6", "del18")


@functools.lru_cache(maxsize=None)
def oracle_data(name, si, mode, base, rule="cut", id0=0, n=N):
    """{t: (labels [n, nodes], stats [n])} of n oracle chains from start plan ``si``, run in
    segments with the stats carried over (the same trajectories as one run of t steps)."""
    g, k, (lo, hi), _, flags = LC.graph_case(name)
    x0 = np.array(LC.start_plans(name)[si], np.int16)
    thr = LC.thr_table(name, base, rule)
    fl = flags if rule == "boundary" else None
    steps = LC.STEPS[name]
    labs = {t: np.empty((n, g.n), np.int16) for t in steps}
    sts = {t: O.new_stats(n) for t in steps}
    for i in range(n):
        lab, st, done = x0, O.new_stats(1), 0
        for t in steps:
            lab, st, _, _ = O.run_chain(g, lab, k, LC.MODE_ID[mode], lo, hi, thr, SEED, id0 + i,
                                        t - done, stats=st, accept_rule=LC.RULE_ID[rule], flags=fl)
            done = t
            labs[t][i] = lab
            sts[t][i] = st[0]
    return {t: (labs[t], sts[t]) for t in steps}


@pytest.mark.parametrize("name", GRAPHS + ("hub5",))
def test_start_plans_exercise_every_branch(name):
    """From the reference alone: over the start plans of a graph some pair fails the
    population bound, some fails contiguity, some cut-edge multiplicity exceeds 1, dcut takes a
    negative, a zero and a positive value, and |B'| != |B| for some pair.  (From the stripe
    seed alone ``pairs`` and ``cutedge`` would share their one-step row.)"""
    plans = LC.start_plans(name)
    assert len(set(plans)) >= 3
    props = LC.start_plan_properties(name)
    assert props["pop_fail"] and props["contig_fail"] and props["multi_edge"]
    assert props["dcut"] == {-1, 0, 1} and props["bratio_changes"]
    if name in ("g4x4", "g3x5"):
        rows = [[LC.chain_law(name, m, MU).row(x) for m in ("pairs", "cutedge")] for x in plans]
        assert any(a != b for a, b in rows)  # the two proposals differ from some start plan
    if name in ("g4x4", "del18"):  # the start plans the boundary rule runs from
        share = LC.boundary_reject_share(name, plans[1:])
        print(f"{name}: the boundary rule rejects {share:.2f} of the valid pairs")
        assert 0.1 <= share <= 0.9


CUT_CASES = [(name, mode, base, si) for name in GRAPHS
             for mode in (("bi", "pairs", "cutedge") if name == "g4x4" else ("pairs", "cutedge"))
             for base in LC.BASES for si in range(3)]


@pytest.mark.parametrize("name,mode,base,si", CUT_CASES,
                         ids=[f"{n}-{m}-{b:.3g}-s{s}" for n, m, b, s in CUT_CASES])
def test_oracle_follows_the_exact_law(name, mode, base, si):
    """cut_accept: plans and counters of 20,000 oracle chains after every t of the graph
    (law_cases.STEPS) from each start plan, both proposals (``bi`` too on k = 2), bases 0.5
    and MU."""
    L = LC.chain_law(name, mode, base)
    x0 = LC.start_plans(name)[si]
    for t, (labels, stats) in oracle_data(name, si, mode, base).items():
        LC.check_law(L, x0, t, labels, stats, f"{name} {mode} {base:.3g} s{si}")


RULE_CASES = [(name, rule, mode, si) for name in ("g4x4", "del18") for rule in ("bratio", "boundary")
              for mode in ("pairs", "cutedge") for si in (1, 2)]


@pytest.mark.parametrize("name,rule,mode,si", RULE_CASES,
                         ids=[f"{n}-{r}-{m}-s{s}" for n, r, m, s in RULE_CASES])
def test_oracle_follows_the_exact_law_under_other_accept_rules(name, rule, mode, si):
    """The |B'| / |B| rule (|B'| recounted from scratch on the proposed plan) and the
    boundary_condition rule (accept iff the flagged nodes of the proposed plan span two
    districts: two neighbouring flagged nodes, so the rule rejects with real mass), at every t
    of the graph."""
    L = LC.chain_law(name, mode, MU, rule)
    x0 = LC.start_plans(name)[si]
    for t, (labels, stats) in oracle_data(name, si, mode, MU, rule).items():
        LC.check_law(L, x0, t, labels, stats, f"{name} {rule} {mode} s{si}")


BURN_IN = {"pairs": 629, "cutedge": 800}


@pytest.mark.parametrize("mode", ["pairs", "cutedge"])
def test_oracle_reaches_the_stationary_law(mode):
    """4 x 4, k = 2, base MU, from the stripe seed: after a burn-in of T steps the plans of
    20,000 chains follow the left eigenvector pi of the full 676-plan matrix.  T is the
    smallest number of steps with || P^T(x0, .) - pi ||_TV <= 1e-3, derived from the reference
    alone (far below what 20,000 chains resolve): T = 629 under ``pairs``, T = 800 under
    ``cutedge`` (BURN_IN; the test re-derives and compares it).  Under ``pairs`` pi(x) is
    proportional to V(x) base^-cut(x), V the number of valid pairs: not the plain Boltzmann
    law (law_ref.ChainLaw.stationary asserts both)."""
    g, k, (lo, hi), seed, _ = LC.graph_case("g4x4")
    L = LC.chain_law("g4x4", mode, MU)
    T, pi = L.burn_in(seed)
    print(f"stationary {mode}: {len(pi)} plans, burn-in T = {T}")
    assert len(pi) == 676 and T == BURN_IN[mode]
    thr = LC.thr_table("g4x4", MU)
    labels = np.stack([O.run_chain(g, seed, k, LC.MODE_ID[mode], lo, hi, thr, SEED + 1, i, T)[0]
                       for i in range(N)])
    stat, dof, p = law_ref.chi2_gof(LC.keyed(pi), LC.count_plans(labels), N)
    print(f"stationary {mode}: chi2 {stat:.1f} / {dof} dof, p = {p:.3g}")
    assert p >= P_MIN


# variant -> (graph, mode, base, start plan, t): the case that rejects it, found by running
# every CUT_CASE against every variant once
TEETH = {"count_invalid": ("g3x5", "pairs", 0.5, 1, 4),
         "swap_weights": ("g3x5", "cutedge", 0.5, 2, 4),
         "flip_dcut": ("g4x4", "pairs", MU, 1, 4),
         "node_then_target": ("g3x5", "pairs", 0.5, 2, 4),
         "no_reyield": ("g4x4", "pairs", MU, 0, 12)}


@pytest.mark.parametrize("variant", list(TEETH))
def test_wrong_laws_are_rejected(variant):
    """Each deliberately wrong law is rejected on the oracle data the true law passes on:
    goodness of fit p < 1e-12 (an observed plan outside the wrong law's support counts), or for
    (e), whose rows are the true ones, |z| > 8 on the yield sums."""
    name, mode, base, si, t = TEETH[variant]
    W = LC.chain_law(name, mode, base, "cut", variant)
    x0 = LC.start_plans(name)[si]
    labels, stats = oracle_data(name, si, mode, base)[t]
    if variant == "no_reyield":
        tot, _ = W.step_moments(x0, t)
        zs = {f: law_ref.moment_z(stats[f], tot[f]) for f in ("sum_cut", "sum_bnodes", "sum_invb")}
        print(f"{variant}: z = {zs}")
        assert max(abs(z) for z in zs.values()) > 8.0
        return
    stat, dof, p = law_ref.chi2_gof(LC.keyed(W.law(x0, t)), LC.count_plans(labels), N,
                                    tail_max=1.0, strict=False)
    tot, _ = W.step_moments(x0, t)
    z_att = law_ref.moment_z(stats["attempts"], tot["attempts"])
    print(f"{variant}: chi2 {stat:.1f} / {dof} dof, p = {p:.3g}; z(attempts) = {z_att:+.1f}")
    assert p < 1e-12
    if variant == "count_invalid":
        assert abs(z_att) > 8.0


@pytest.mark.parametrize("mode", ["pairs", "cutedge"])
@pytest.mark.parametrize("si", [0, 1, 2])
def test_halves_of_the_chain_id_range_are_independent_samples(mode, si):
    """4 x 4 at t = 1: the even and the odd chain ids, and the low and the high half of the
    range, each pass the goodness of fit on their own, and the 2 x cells contingency test
    between the halves has p >= 1e-6 (a Philox counter layout that correlates neighbouring
    chain ids, or one that repeats with the id's high bits, would fail here)."""
    L = LC.chain_law("g4x4", mode, MU)
    x0 = LC.start_plans("g4x4")[si]
    law = LC.keyed(L.law(x0, 1))
    labels, _ = oracle_data("g4x4", si, mode, MU)[1]
    for what, a, b in (("even/odd", labels[0::2], labels[1::2]),
                       ("low/high", labels[:N // 2], labels[N // 2:])):
        ca, cb = LC.count_plans(a), LC.count_plans(b)
        pa = law_ref.chi2_gof(law, ca, len(a))[2]
        pb = law_ref.chi2_gof(law, cb, len(b))[2]
        stat, dof, pc = law_ref.contingency(law, ca, cb)
        print(f"{mode} s{si} {what}: p = {pa:.3g}, {pb:.3g}; contingency {stat:.1f} / {dof}, "
              f"p = {pc:.3g}")
        assert min(pa, pb, pc) >= P_MIN


def test_tempered_oracle_follows_the_exact_joint_law():
    """16,384 two-rung replica sets through ladder_ref.tempered_ref (with 5,000 sets the pooled
    tail of the exact joint law holds 35% of it and the goodness of fit allows 20%; 16,384 is
    the smallest power of two that meets the condition): the pair (plan on rung 0,
    plan on rung 1) after two rounds of two steps against the exact joint law built from the
    law_ref rows and the swap probability min(1, (b0 / b1)^(cut0 - cut1)), and each rung's
    marginal against the exact marginal."""
    from flipcomplexityempirical_amd.chain import ladder_layout
    from ladder_ref import tempered_ref
    g, k, bounds, seed, joint = LC.tempered_case()
    n_sets = 16384
    s, r = ladder_layout(2 * n_sets, 2)
    ref = tempered_ref(g, seed, k, 1, bounds, (0.5, MU), s, r, SEED + 2, 0, 2, 2)
    rs = ref["rung_stats"]
    assert 0 < rs["swap_done"].sum() < rs["swap_tried"].sum()
    LC.check_tempered(joint, ref["labels"], ref["rungs"], n_sets, "host ladder")
