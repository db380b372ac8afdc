"""The exact law of one counted step of the flip chain, derived independently of the oracle.

Plain Python over a networkx graph built from ``Graph.rowptr / col``: no oracle code, no
ctypes, no Philox.  A plan is a tuple of district labels, one per node.  What a counted step
does (include/flipwalk.h, oracle/flipchain_oracle.c header):

* a proposal is drawn from the proposal set of the current plan: every (node, distinct foreign
  neighbouring district) pair with weight 1 under ``bi`` / ``pairs``; under ``cutedge`` the
  pair's weight is the number of the node's neighbours in that district (a uniform directed
  cut edge);
* an invalid proposal (population bound first, then contiguity of the source district without
  the node) is retried without being counted, so the counted proposal is the proposal law
  conditioned on validity;
* the valid proposal is accepted with the probability of the accept rule, else the chain
  stays where it is, and either way one state is yielded.

``variant=`` produces deliberately wrong laws, for the tests that show the checks have teeth:

  "count_invalid"     (a) an invalid proposal counts as a step and stays put
  "swap_weights"      (b) ``pairs`` draws by cut-edge weight and ``cutedge`` by pair
  "flip_dcut"         (c) the sign of dcut is flipped in the accept bound
  "node_then_target"  (d) uniform over boundary nodes, then uniform over the node's targets
  "no_reyield"        (e) a rejected step yields nothing (moments only; the rows are the true ones)
"""
from __future__ import annotations

import math
from collections import defaultdict

import networkx as nx
import numpy as np

MODES = {0: "bi", 1: "pairs", 2: "cutedge", "bi": "bi", "pairs": "pairs", "cutedge": "cutedge"}
RULES = {0: "cut", 1: "bratio", 2: "boundary", "cut": "cut", "bratio": "bratio",
         "boundary": "boundary"}
VARIANTS = (None, "count_invalid", "swap_weights", "flip_dcut", "node_then_target", "no_reyield")
COUNTERS = ("attempts", "pop_fail", "contig_fail", "accepts", "sum_deg", "acc_deg", "sum_cut",
            "sum_bnodes", "sum_invb")


def nx_graph(graph):
    G = nx.Graph()
    G.add_nodes_from(range(graph.n))
    for v in range(graph.n):
        for u in graph.col[graph.rowptr[v]:graph.rowptr[v + 1]]:
            G.add_edge(v, int(u))
    return G


def plan_of(labels):
    return tuple(int(x) for x in labels)


class ChainLaw:
    """The chain of one configuration; rows and per-plan moments are cached."""

    def __init__(self, graph, k, mode, lo, hi, thr_or_base, accept_rule="cut", flags=None,
                 variant=None):
        assert variant in VARIANTS
        self.G = nx_graph(graph)
        self.n, self.k = graph.n, int(k)
        self.nbrs = [sorted(self.G[v]) for v in range(self.n)]
        self.deg = [len(x) for x in self.nbrs]
        self.maxdeg = max(self.deg)
        self.pop = [int(p) for p in graph.pop_array()]
        self.mode, self.rule = MODES[mode], RULES[accept_rule]
        self.lo, self.hi = int(lo), int(hi)
        if np.ndim(thr_or_base) == 0:
            self.base, self.thr = float(thr_or_base), None
        else:
            self.base, self.thr = None, [float(x) for x in thr_or_base]
            assert len(self.thr) == 2 * self.maxdeg + 1
        self.flags = None if flags is None else [bool(f) for f in flags]
        assert self.rule != "boundary" or self.flags is not None
        self.variant = variant
        self._connected, self._proposals, self._rows, self._moments = {}, {}, {}, {}

    # ------------------------------------------------------------------ pieces
    def bound(self, dcut):
        if self.variant == "flip_dcut":
            dcut = -dcut
        return self.thr[dcut + self.maxdeg] if self.thr is not None else self.base ** (-dcut)

    def cut(self, plan):
        return sum(1 for u, w in self.G.edges if plan[u] != plan[w])

    def boundary(self, plan):
        """|B|: nodes with a neighbour in another district (b_nodes_bi)."""
        return sum(1 for v in range(self.n) if any(plan[u] != plan[v] for u in self.nbrs[v]))

    def connected_without(self, plan, a, v):
        nodes = [u for u in range(self.n) if plan[u] == a and u != v]
        if not nodes:
            return False
        key = sum(1 << u for u in nodes)
        hit = self._connected.get(key)
        if hit is None:
            hit = self._connected[key] = nx.is_connected(self.G.subgraph(nodes))
        return hit

    def accept_prob(self, plan, nxt, dcut):
        if self.rule == "cut":
            return min(1.0, self.bound(dcut))
        if self.rule == "bratio":
            return min(1.0, self.bound(dcut) * self.boundary(nxt) / self.boundary(plan))
        parts = {nxt[v] for v in range(self.n) if self.flags[v]}
        return 1.0 if len(parts) >= 2 else 0.0

    def proposals(self, plan):
        """Every proposal of ``plan``: (v, target, weight, verdict, dcut, next plan, accept
        probability); verdict is "ok", "pop" or "contig" (the population check comes first)."""
        hit = self._proposals.get(plan)
        if hit is not None:
            return hit
        pops = [0] * self.k
        for v in range(self.n):
            pops[plan[v]] += self.pop[v]
        mode = self.mode
        if self.variant == "swap_weights":
            mode = "cutedge" if mode != "cutedge" else "pairs"
        nb = self.boundary(plan)
        out = []
        for v in range(self.n):
            a = plan[v]
            count = defaultdict(int)
            for u in self.nbrs[v]:
                count[plan[u]] += 1
            na = count.pop(a, 0)
            for b in sorted(count):
                if self.variant == "node_then_target":
                    w = 1.0 / (nb * len(count))
                else:
                    w = float(count[b]) if mode == "cutedge" else 1.0
                dcut = na - count[b]
                if pops[a] - self.pop[v] < self.lo or pops[b] + self.pop[v] > self.hi:
                    out.append((v, b, w, "pop", dcut, None, 0.0))
                elif not self.connected_without(plan, a, v):
                    out.append((v, b, w, "contig", dcut, None, 0.0))
                else:
                    nxt = plan[:v] + (b,) + plan[v + 1:]
                    out.append((v, b, w, "ok", dcut, nxt, self.accept_prob(plan, nxt, dcut)))
        self._proposals[plan] = out
        return out

    # ------------------------------------------------------------------ rows
    def row(self, plan):
        """{next plan: probability} of one counted step from ``plan``."""
        hit = self._rows.get(plan)
        if hit is not None:
            return hit
        props = self.proposals(plan)
        valid = sum(p[2] for p in props if p[3] == "ok")
        assert valid > 0, ("no valid proposal: the chain is stuck", plan)
        norm = sum(p[2] for p in props) if self.variant == "count_invalid" else valid
        row = defaultdict(float)
        moved = 0.0
        for v, b, w, verdict, dcut, nxt, pa in props:
            if verdict == "ok" and pa > 0.0:
                row[nxt] += w / norm * pa
                moved += w / norm * pa
        if 1.0 - moved > 0.0:  # rejected (and, under (a), invalid) mass stays
            row[plan] += 1.0 - moved
        row = self._rows[plan] = dict(row)
        return row

    def moments(self, plan):
        """Exact conditional expectations of one counted step given the current plan."""
        hit = self._moments.get(plan)
        if hit is not None:
            return hit
        props = self.proposals(plan)
        tot = sum(p[2] for p in props)
        ok = [p for p in props if p[3] == "ok"]
        valid = sum(p[2] for p in ok)
        m = {"attempts": tot / valid,
             "pop_fail": sum(p[2] for p in props if p[3] == "pop") / valid,
             "contig_fail": sum(p[2] for p in props if p[3] == "contig") / valid,
             "accepts": sum(p[2] * p[6] for p in ok) / valid,
             # the node's degree summed over every attempt of the step, and over accepts
             "sum_deg": sum(p[2] * self.deg[p[0]] for p in props) / valid,
             "acc_deg": sum(p[2] * p[6] * self.deg[p[0]] for p in ok) / valid,
             "cut": self.cut(plan), "bnodes": self.boundary(plan)}
        if self.variant == "count_invalid":
            m.update(attempts=1.0, pop_fail=m["pop_fail"] * valid / tot,
                     contig_fail=m["contig_fail"] * valid / tot, accepts=m["accepts"] * valid / tot,
                     sum_deg=m["sum_deg"] * valid / tot, acc_deg=m["acc_deg"] * valid / tot)
        # the state an accepted step yields (variant (e) yields nothing else)
        m["acc_cut"] = sum(p[2] * p[6] * self.cut(p[5]) for p in ok if p[6] > 0) / valid
        m["acc_bnodes"] = sum(p[2] * p[6] * self.boundary(p[5]) for p in ok if p[6] > 0) / valid
        m["acc_invb"] = sum(p[2] * p[6] / self.boundary(p[5]) for p in ok if p[6] > 0) / valid
        self._moments[plan] = m
        return m

    def step(self, vec):
        out = defaultdict(float)
        for x, p in vec.items():
            for y, q in self.row(x).items():
                out[y] += p * q
        return dict(out)

    def law(self, x0, t):
        """P^t(x0, .): only the plans reachable in t steps are expanded."""
        vec = {plan_of(x0): 1.0}
        for _ in range(int(t)):
            vec = self.step(vec)
        return vec

    def step_moments(self, x0, T):
        """Exact expectations after T counted steps from x0.  Returns (totals, per_yield):
        totals[name] for the COUNTERS (E[attempts], E[pop_fail], E[contig_fail], E[accepts],
        E[sum_deg], E[acc_deg] as sums over the steps' conditional expectations under
        P^s(x0, .), s < T; E[sum_cut], E[sum_bnodes], E[sum_invb] as sums over the yields
        0..T, the initial state yielded once and a rejected step re-yielding), and per_yield =
        {"cut", "bnodes", "invb"}: the expectation of the state at each yield index."""
        vec = {plan_of(x0): 1.0}
        tot = dict.fromkeys(COUNTERS, 0.0)
        per = {"cut": [], "bnodes": [], "invb": []}
        for s in range(int(T) + 1):
            ms = [(p, self.moments(x)) for x, p in vec.items()]
            per["cut"].append(sum(p * m["cut"] for p, m in ms))
            per["bnodes"].append(sum(p * m["bnodes"] for p, m in ms))
            per["invb"].append(sum(p / m["bnodes"] for p, m in ms))
            if self.variant != "no_reyield" or s == 0:
                tot["sum_cut"] += per["cut"][-1]
                tot["sum_bnodes"] += per["bnodes"][-1]
                tot["sum_invb"] += per["invb"][-1]
            if s == T:
                break
            for name in ("attempts", "pop_fail", "contig_fail", "accepts", "sum_deg", "acc_deg"):
                tot[name] += sum(p * m[name] for p, m in ms)
            if self.variant == "no_reyield":
                tot["sum_cut"] += sum(p * m["acc_cut"] for p, m in ms)
                tot["sum_bnodes"] += sum(p * m["acc_bnodes"] for p, m in ms)
                tot["sum_invb"] += sum(p * m["acc_invb"] for p, m in ms)
            vec = self.step(vec)
        return tot, per

    # ------------------------------------------------------------------ the whole state space
    def closure(self, x0):
        """Every plan reachable from x0, in discovery order."""
        x0 = plan_of(x0)
        seen, todo = {x0: 0}, [x0]
        while todo:
            x = todo.pop()
            for y in self.row(x):
                if y not in seen:
                    seen[y] = len(seen)
                    todo.append(y)
        return list(seen)

    def matrix(self, x0):
        states = self.closure(x0)
        idx = {x: i for i, x in enumerate(states)}
        P = np.zeros((len(states), len(states)))
        for x, i in idx.items():
            for y, q in self.row(x).items():
                P[i, idx[y]] += q
        assert np.abs(P.sum(1) - 1.0).max() < 1e-12
        return states, P

    def stationary(self, x0):
        """(states, pi, P): the left eigenvector of the full matrix over the plans reachable
        from x0, pi P = pi to 1e-12.

        What the stationary law is.  The proposal is uniform over the VALID pairs of the
        current plan x, V(x) of them, not over a set of the same size everywhere, and the
        accept step min(1, base^-dcut) does not correct for that.  Under ``bi`` / ``pairs``
        every valid move x -> y has the valid reverse move y -> x (the districts of x are
        connected and inside the bounds), so  pi(x) / V(x) * min(1, base^(cut x - cut y))  is
        symmetric in x and y exactly when pi(x) is proportional to V(x) * base^-cut(x): the
        chain is reversible with respect to  pi(x) ~ V(x) base^-cut(x),  NOT the plain
        Boltzmann law base^-cut(x); pi(x) / V(x) is proportional to base^-cut(x), pi(x) itself
        is not.  Asserted below against the eigenvector.  Under ``cutedge`` the move x -> y has
        weight (neighbours of v in the target) and its reverse (neighbours of v in the
        source), which no function of the plan balances in general: no closed form is claimed
        there, and the eigenvector alone is the reference."""
        states, P = self.matrix(x0)
        n = len(states)
        A = P.T - np.eye(n)
        A[-1, :] = 1.0
        rhs = np.zeros(n)
        rhs[-1] = 1.0
        pi = np.linalg.solve(A, rhs)
        for _ in range(3):
            pi = pi @ P
            pi /= pi.sum()
        assert pi.min() > 0 and np.abs(pi @ P - pi).max() < 1e-12
        if self.mode != "cutedge" and self.rule == "cut" and self.variant is None:
            V = np.array([sum(1 for p in self.proposals(x) if p[3] == "ok") for x in states], float)
            cut = np.array([self.cut(x) for x in states], float)
            base = self.base if self.base is not None else 1.0 / self.thr[self.maxdeg + 1]
            want = V * base ** (-cut)
            want /= want.sum()
            assert np.abs(pi / want - 1.0).max() < 1e-9, "pi is not V(x) base^-cut(x)"
            if V.min() != V.max() and base != 1.0:
                boltz = base ** (-cut)
                boltz /= boltz.sum()
                assert np.abs(pi / boltz - 1.0).max() > 1e-3, "pi equals the plain Boltzmann law"
        return states, pi, P

    def burn_in(self, x0, tv=1e-3, t_max=100000):
        """The smallest T with total-variation distance || P^T(x0, .) - pi || <= tv."""
        states, pi, P = self.stationary(x0)
        vec = np.zeros(len(states))
        vec[states.index(plan_of(x0))] = 1.0
        for T in range(t_max + 1):
            if 0.5 * np.abs(vec - pi).sum() <= tv:
                return T, dict(zip(states, pi))
            vec = vec @ P
        raise AssertionError("no burn-in found")


def tempered_joint(rung0, rung1, x0, steps_per_round, n_rounds, round0=0):
    """The exact joint law {(plan on rung 0, plan on rung 1): p} of one two-rung replica set
    after n_rounds x (steps_per_round steps of each chain under its rung's ChainLaw, one
    exchange).  Round r tries the pairs range(r & 1, n_rungs - 1, 2) (ladder_ref.exchange_ref,
    include/flipwalk.h): with two rungs, the pair (0, 1) on even rounds and none on odd ones;
    it swaps with probability min(1, (b0 / b1) ^ (cut0 - cut1))."""
    x0 = plan_of(x0)
    joint = {(x0, x0): 1.0}
    ratio = rung0.base / rung1.base
    for r in range(round0, round0 + int(n_rounds)):
        for _ in range(int(steps_per_round)):
            half = defaultdict(float)
            for (x, y), p in joint.items():
                for x2, q in rung0.row(x).items():
                    half[(x2, y)] += p * q
            joint = defaultdict(float)
            for (x, y), p in half.items():
                for y2, q in rung1.row(y).items():
                    joint[(x, y2)] += p * q
        if 0 in range(r & 1, 1, 2):
            out = defaultdict(float)
            for (x, y), p in joint.items():
                a = min(1.0, ratio ** (rung0.cut(x) - rung1.cut(y)))
                out[(y, x)] += p * a
                if a < 1.0:
                    out[(x, y)] += p * (1.0 - a)
            joint = out
    return dict(joint)


def marginal(joint, axis):
    out = defaultdict(float)
    for key, p in joint.items():
        out[key[axis]] += p
    return dict(out)


# ---------------------------------------------------------------------- plain function calls
def transition_row(graph, plan, k, mode, lo, hi, thr_or_base, accept_rule="cut", flags=None,
                   variant=None):
    return ChainLaw(graph, k, mode, lo, hi, thr_or_base, accept_rule, flags, variant).row(
        plan_of(plan))


def law(graph, k, mode, lo, hi, thr_or_base, x0, t, accept_rule="cut", flags=None, variant=None):
    return ChainLaw(graph, k, mode, lo, hi, thr_or_base, accept_rule, flags, variant).law(x0, t)


def step_moments(graph, k, mode, lo, hi, thr_or_base, x0, T, accept_rule="cut", flags=None,
                 variant=None):
    return ChainLaw(graph, k, mode, lo, hi, thr_or_base, accept_rule, flags,
                    variant).step_moments(x0, T)


def stationary(graph, k, mode, lo, hi, thr_or_base, x0, accept_rule="cut", flags=None):
    return ChainLaw(graph, k, mode, lo, hi, thr_or_base, accept_rule, flags).stationary(x0)


# ---------------------------------------------------------------------- statistics
class ImpossiblePlan(AssertionError):
    """A plan was observed that the exact law gives probability 0."""


def pooled_cells(law, n, tail_max=0.2):
    """Cochran's rule: the plans with expectation n p >= 5 are cells of their own, in a fixed
    order; all others form one tail cell.  The tail's exact share must be <= tail_max: a
    condition on the reference and n alone, asserted here.  A tail whose own expectation is
    below 5 joins the smallest kept cell.  Returns (plans of the kept cells, expectations with
    the tail last when there is one, index of the cell the tail joined or None)."""
    total = math.fsum(law.values())
    assert abs(total - 1.0) < 1e-9, total
    keep = sorted((x for x, p in law.items() if n * p >= 5.0), key=lambda x: (-law[x], x))
    assert keep, "no cell reaches expectation 5"
    exp = [n * law[x] for x in keep]
    tail = max(0.0, 1.0 - math.fsum(law[x] for x in keep))
    assert tail <= tail_max, f"pooled tail holds {tail:.3f} of the law (> {tail_max})"
    joined = None
    if n * tail >= 5.0:
        exp.append(n * tail)
    elif n * tail > 1e-9:
        joined = len(keep) - 1
        exp[joined] += n * tail
    return keep, np.array(exp), joined


def cell_counts(keep, n_cells, joined, counts):
    idx = {x: i for i, x in enumerate(keep)}
    tail_to = n_cells - 1 if joined is None else joined
    obs = np.zeros(n_cells)
    for x, c in counts.items():
        obs[idx.get(x, tail_to)] += c
    return obs


def chi2_gof(law, counts, n, tail_max=0.2, strict=True):
    """Chi-square goodness of fit of observed plan counts to the exact law.  A plan observed
    with exact probability 0 is a hard failure on its own (ImpossiblePlan, naming the plan;
    with strict=False: p = 0).  Returns (stat, dof, p)."""
    from scipy.stats import chi2
    assert sum(counts.values()) == n
    for x in counts:
        if law.get(x, 0.0) <= 0.0:
            if strict:
                raise ImpossiblePlan(f"observed {counts[x]} x a plan of probability 0: {x}")
            return math.inf, 0, 0.0
    keep, exp, joined = pooled_cells(law, n, tail_max)
    obs = cell_counts(keep, len(exp), joined, counts)
    stat = float(((obs - exp) ** 2 / exp).sum())
    dof = len(exp) - 1
    if dof == 0:
        return stat, 0, 1.0
    return stat, dof, float(chi2.sf(stat, dof))


def chi2_z(stat, dof):
    """The chi-square statistic as a z-score (for reports)."""
    return (stat - dof) / math.sqrt(2.0 * dof) if dof else 0.0


def contingency(law, counts_a, counts_b, tail_max=0.2):
    """2 x cells test of homogeneity between two samples, on the cells the exact law gives the
    smaller sample.  Returns (stat, dof, p)."""
    from scipy.stats import chi2_contingency
    na, nb = sum(counts_a.values()), sum(counts_b.values())
    keep, exp, joined = pooled_cells(law, min(na, nb), tail_max)
    table = np.stack([cell_counts(keep, len(exp), joined, c) for c in (counts_a, counts_b)])
    table = table[:, table.sum(0) > 0]
    if table.shape[1] < 2:
        return 0.0, 0, 1.0
    stat, p, dof, _ = chi2_contingency(table, correction=False)
    return float(stat), int(dof), float(p)


def moment_z(values, expected):
    """z of the across-chain mean against its exact expectation, the standard error from the
    across-chain sample variance.  A counter that is constant across the chains must equal
    its expectation (to rounding); then z = 0, else +-inf."""
    v = np.asarray(values, np.float64)
    mean, sd = float(v.mean()), float(v.std(ddof=1))
    if sd == 0.0:
        return 0.0 if abs(mean - expected) <= 1e-9 * max(1.0, abs(expected)) else math.inf
    return (mean - expected) / (sd / math.sqrt(len(v)))
