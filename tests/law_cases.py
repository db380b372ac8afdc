"""Graphs, start plans and cached exact laws shared by test_law_host.py and test_gpu_law.py.

The start plans are chosen by walking the reference's own state graph (law_ref rows at base 1)
with a fixed ``random.Random``; nothing here touches the oracle or the kernels.
"""
from __future__ import annotations

import functools
import random

import networkx as nx
import numpy as np

import law_ref
from cases import MU
from flipcomplexityempirical_amd.chain import annealing_table, population_bounds
from flipcomplexityempirical_amd.graph import (Graph, band_seed, block_seed, delaunay_graph,
                                               grid_graph, stripe_seed)
from flipcomplexityempirical_amd.seeds import tree_seed

BASES = (0.5, MU)
# Steps per graph: {1, 4, 12}, and 25 on 4 x 4, except where the reference alone rules the
# larger t out.  From the walked start plans the 4 x 6, k = 4 law reaches 6,529 plans at t = 6
# already, with 24-36% of its mass in cells expecting fewer than 5 of 20,000 chains (the
# pooled-tail condition allows 20%), and the 18-node Delaunay law at t = 12 spreads over
# ~270,000 plans (48-72% pooled, 15-35 s to build); both stop at t = 4.  The hub graphs stop at
# t = 2, which keeps their references small.
STEPS = {"g4x4": (1, 4, 12, 25), "g3x5": (1, 4, 12), "g5x3": (1, 4, 12), "g4x6": (1, 4),
         "del18": (1, 4), "hub5": (1, 2), "hub14": (1, 2)}
MODE_ID = {"bi": 0, "pairs": 1, "cutedge": 2}
RULE_ID = {"cut": 0, "bratio": 1, "boundary": 2}


def hub5_graph(degree: int = 18) -> Graph:
    """A 5 x 5 grid plus one hub joined to ``degree`` cells, after ``cases.hub_graph``.  Degree
    18 > 16: no padded-row table, the CSR-walking kernel.  Degree 14 with k = 2: padded rows,
    and k + maxdeg = 16 needs the 8-bit in-place label codes."""
    G = nx.grid_2d_graph(5, 5)
    G.add_node("hub")
    cells = [(r, c) for r in range(5) for c in range(5)]
    for rc in cells[3:3 + degree]:
        G.add_edge("hub", rc)
    for v in G.nodes:
        G.nodes[v]["boundary_node"] = isinstance(v, tuple) and (min(v) == 0 or max(v) == 4)
    return Graph.from_networkx(G)


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """(graph, k, (lo, hi), seed plan, boundary flags)."""
    if name == "g4x4":
        g, k, pct, seed = grid_graph(4, 4), 2, 0.3, stripe_seed(4, 4)
    elif name == "g3x5":
        g, k, pct, seed = grid_graph(3, 5), 3, 0.5, band_seed(3, 5, 3)
    elif name == "g5x3":  # width 3: below the grid kernel's narrowest
        g, k, pct, seed = grid_graph(5, 3), 3, 0.5, band_seed(5, 3, 3)
    elif name == "g4x6":
        g, k, pct, seed = grid_graph(4, 6), 4, 0.2, block_seed(4, 6, 2, 2)
    elif name == "del18":
        g, k, pct = delaunay_graph(18, seed=3, pop_sigma=0.3), 3, 0.4
        seed = tree_seed(g, k, pct)
    elif name == "hub5":
        g, k, pct = hub5_graph(), 2, 0.3
        seed = tree_seed(g, k, pct)
    elif name == "hub14":
        g, k, pct = hub5_graph(14), 2, 0.3
        seed = tree_seed(g, k, pct)
    else:
        raise KeyError(name)
    # boundary_condition flags: two neighbouring nodes, so that from the start plans the flagged
    # nodes often lie in one district and the rule rejects with real mass (the grid's outer
    # ring would span both districts of every reachable 4 x 4 plan and never reject)
    flagged = {"del18": (7, 16)}.get(name, (g.grid_w + 1, g.grid_w + 2) if g.grid_w else (0, 1))
    flags = np.isin(np.arange(g.n), flagged).astype(np.uint8)
    return g, k, population_bounds(g.total_pop, k, pct), np.asarray(seed, np.int16), flags


_LAWS = {}


def chain_law(name, mode, base, rule="cut", variant=None):
    """The cached exact chain (rows are kept across tests: a module-level cache)."""
    key = (name, mode, base, rule, variant)
    if key not in _LAWS:
        g, k, (lo, hi), _, flags = graph_case(name)
        _LAWS[key] = law_ref.ChainLaw(g, k, mode, lo, hi, float(base), rule,
                                      flags if rule == "boundary" else None, variant)
    return _LAWS[key]


def thr_table(name, base, rule="cut"):
    """The bound table handed to the oracle and the kernels: base^-d, and for the |B'|/|B|
    rule base^(beta * -d) with beta = 1 (the same numbers)."""
    g = graph_case(name)[0]
    return annealing_table(base, 1, g.maxdeg)


@functools.lru_cache(maxsize=None)
def start_plans(name, n_plans=3, stride=7):
    """The seed plan and plans met every ``stride`` moves of a fixed random walk over the
    reference's state graph (``pairs`` rows at base 1)."""
    seed = law_ref.plan_of(graph_case(name)[3])
    walk = chain_law(name, "pairs", 1.0)
    rng = random.Random(20241021)
    plans, x = [seed], seed
    while len(plans) < n_plans:
        for _ in range(stride):
            x = rng.choice(sorted(y for y in walk.row(x) if y != x))
        if x not in plans:
            plans.append(x)
    return tuple(plans)


def start_plan_properties(name, plans=None):
    """What the start plans' proposal sets contain, from the reference alone."""
    pairs = chain_law(name, "pairs", 1.0)
    cutedge = chain_law(name, "cutedge", 1.0)
    out = {"pop_fail": False, "contig_fail": False, "multi_edge": False, "dcut": set(),
           "bratio_changes": False}
    for x in plans or start_plans(name):
        for v, b, w, verdict, dcut, nxt, _ in pairs.proposals(x):
            out["pop_fail"] |= verdict == "pop"
            out["contig_fail"] |= verdict == "contig"
            if verdict == "ok":
                out["dcut"].add((dcut > 0) - (dcut < 0))
                out["bratio_changes"] |= pairs.boundary(nxt) != pairs.boundary(x)
        out["multi_edge"] |= any(p[2] > 1 for p in cutedge.proposals(x))
    return out


def boundary_reject_share(name, plans):
    """The share of the valid ``pairs`` proposals of ``plans`` that the boundary rule rejects
    (accept probability 0), from the reference alone."""
    L = chain_law(name, "pairs", MU, "boundary")
    ok = [p for x in plans for p in L.proposals(x) if p[3] == "ok"]
    return sum(1 for p in ok if p[6] == 0.0) / len(ok)


def plan_key(plan):
    return np.asarray(plan, np.int16).tobytes()


def keyed(law):
    """The law keyed by the int16 bytes of the plan, as label rows are counted."""
    return {plan_key(x): p for x, p in law.items()}


def count_plans(labels):
    """{bytes of the plan: count} over the rows of an int16 label array."""
    lab = np.ascontiguousarray(labels, np.int16)
    rows, cnt = np.unique(lab, axis=0, return_counts=True)
    return {r.tobytes(): int(c) for r, c in zip(rows, cnt)}


P_MIN, Z_MAX = 1e-6, 5.0
TEMPERED_START = (0, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1)


def check_law(L, x0, t, labels, stats, report):
    """The goodness of fit of the plans and the z of every counter; returns (p, max |z|)."""
    n = len(labels)
    stat, dof, p = law_ref.chi2_gof(keyed(L.law(x0, t)), count_plans(labels), n)
    tot, per = L.step_moments(x0, t)
    zs = {name: law_ref.moment_z(stats[name], tot[name]) for name in law_ref.COUNTERS}
    # the state at the last yield: E[cut], E[|B|], E[1/|B|]
    zs["cut"] = law_ref.moment_z(stats["cut"], per["cut"][t])
    zs["bnodes"] = law_ref.moment_z(stats["bnodes"], per["bnodes"][t])
    zs["invb"] = law_ref.moment_z(1.0 / stats["bnodes"], per["invb"][t])
    zmax = max(abs(z) for z in zs.values())
    print(f"{report} t={t}: chi2 {stat:.1f} / {dof} dof, p = {p:.3g}, "
          f"z = {law_ref.chi2_z(stat, dof):+.2f}; max |z| of the counters {zmax:.2f} "
          f"({max(zs, key=lambda k: abs(zs[k]))})")
    assert (stats["yields"] == t + 1).all() and (stats["steps"] == t).all()
    assert not stats["stuck"].any()
    assert p >= P_MIN, (report, t, stat, dof, p)
    assert zmax <= Z_MAX, (report, t, zs)
    return p, zmax


def tempered_case():
    """The two-rung ladder both replica-exchange tests use: 4 x 4, k = 2, ``pairs``, bases
    (0.5, MU), run_tempered(2, 2), every replica set started from TEMPERED_START.  From the
    stripe seed the joint law spreads over 19,881 pairs and its pooled tail holds 22% of it at
    32,768 sets, past the 20% the goodness of fit allows; from this plan (found among the
    reachable plans by that figure alone) it holds 13%."""
    g, k, bounds, _, _ = graph_case("g4x4")
    seed = np.array(TEMPERED_START, np.int16)
    joint = law_ref.tempered_joint(chain_law("g4x4", "pairs", 0.5),
                                   chain_law("g4x4", "pairs", MU), seed, 2, 2)
    return g, k, bounds, seed, joint


def check_tempered(joint, labels, rungs, n_sets, report):
    """labels [2 n_sets, nodes] and rungs [2 n_sets] of consecutive-chain replica sets against
    the exact joint law and both exact marginals."""
    lab = np.asarray(labels, np.int16).reshape(n_sets, 2, -1)
    r = np.asarray(rungs).reshape(n_sets, 2)
    assert (np.sort(r, 1) == [0, 1]).all()
    on0 = np.where((r[:, 0] == 0)[:, None], lab[:, 0], lab[:, 1])
    on1 = np.where((r[:, 0] == 0)[:, None], lab[:, 1], lab[:, 0])
    out = {}
    pairs = {plan_key(x) + plan_key(y): p for (x, y), p in joint.items()}
    for what, law, rows in (("joint", pairs, np.concatenate([on0, on1], 1)),
                            ("rung 0", keyed(law_ref.marginal(joint, 0)), on0),
                            ("rung 1", keyed(law_ref.marginal(joint, 1)), on1)):
        stat, dof, p = law_ref.chi2_gof(law, count_plans(rows), n_sets)
        print(f"{report} {what}: chi2 {stat:.1f} / {dof} dof, p = {p:.3g}")
        out[what] = p
    assert min(out.values()) >= P_MIN, out
    return out
