"""The kernels against the exact law of the chain (law_ref.py), at the C3 chain count.

Every case runs 65,536 chains on a tiny graph (8,192 where the W2 register budget is meant: the
plan takes it only when all the work fits one round): one launch of t steps (unless the case
splits it), then ``labels()`` and ``stats()``.  Every plan must lie in the exact support of
P^t(x0, .), together they must pass the goodness of fit (p >= 1e-6), and every counter's
across-chain mean must sit within |z| <= 5 of its exact expectation: the checks of
test_law_host.py (law_cases.check_law), one or more rows per kernel family.  The first and the
last 64 chains are also compared with the oracle bit for bit, so a law failure can be told from
a parity failure at a glance.  No bit-exact test reaches this chain count.

Each case names the kernel it means and fails when another one ran: the kernel, the rows per
chain and the register budget are read from the library's FLIPWALK_VERBOSE plan line, the label
width from the handle.  The plan line does not tell the lean from the FULL instantiation (the
accept rule selects FULL when the launch is made) nor the padded-row from the CSR-walking
kernel (the graph's maximum degree selects it: above 16 there is no padded-row table); those
two follow from the case's inputs.
"""
import numpy as np
import pytest

import law_cases as LC
from cases import MU
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 65536
SEED = 20241021
KNOBS = ("FLIPWALK_NO_GRID16", "FLIPWALK_NO_BITBOARD", "FLIPWALK_SPEC", "FLIPWALK_W2",
         "FLIPWALK_CSR_LB", "FLIPWALK_GRID_CAP", "FLIPWALK_SLICES", "FLIPWALK_FOLD_AT",
         "FLIPWALK_LAUNCH_STEPS", "FLIPWALK_LIST_CAP", "FLIPWALK_GRID16_NW", "FLIPWALK_NO_ROWBB",
         "FLIPWALK_NO_WB", "FLIPWALK_NO_WPE5")


def grid(rows, w2=False):
    return {"kernel": "grid", "bits": 2, "rows": rows, "w2": w2}


def chain(bits):
    return {"kernel": "chain", "bits": bits}


# (id, graph, proposal, base, accept rule, start plan, launches, knobs, chains, what must run)
FAMILIES = [
    # the four-chains-per-wave grid kernel at W = 4, its narrowest, and on 4 x 6 with k = 4:
    # 1, 2 and 4 rows per chain, the list search, and the W2 register budget
    ("grid-4x4-spec1", "g4x4", "pairs", MU, "cut", 1, (4,), {"FLIPWALK_SPEC": "1", "FLIPWALK_W2": "0"}, N, grid(1)),
    ("grid-4x4-spec2", "g4x4", "cutedge", 0.5, "cut", 2, (12,), {"FLIPWALK_SPEC": "2"}, N, grid(2)),
    ("grid-4x4-spec4", "g4x4", "bi", MU, "cut", 0, (25,), {"FLIPWALK_SPEC": "4"}, N, grid(4)),
    ("grid-4x4-list", "g4x4", "pairs", 0.5, "cut", 2, (1,), {"FLIPWALK_NO_BITBOARD": "1", "FLIPWALK_SPEC": "1", "FLIPWALK_W2": "0"}, N, grid(1)),
    ("grid-4x4-w2", "g4x4", "pairs", MU, "cut", 1, (12,), {"FLIPWALK_SPEC": "1", "FLIPWALK_W2": "1"}, 8192, grid(1, True)),
    ("grid-4x6-spec1", "g4x6", "cutedge", MU, "cut", 1, (4,), {"FLIPWALK_SPEC": "1", "FLIPWALK_W2": "0"}, N, grid(1)),
    ("grid-4x6-spec2", "g4x6", "pairs", 0.5, "cut", 2, (4,), {"FLIPWALK_SPEC": "2"}, N, grid(2)),
    ("grid-4x6-spec4", "g4x6", "pairs", MU, "cut", 0, (1,), {"FLIPWALK_SPEC": "4"}, N, grid(4)),
    ("grid-4x6-list", "g4x6", "cutedge", 0.5, "cut", 1, (4,), {"FLIPWALK_NO_BITBOARD": "1", "FLIPWALK_SPEC": "1", "FLIPWALK_W2": "0"}, N, grid(1)),
    ("grid-4x6-w2", "g4x6", "cutedge", MU, "cut", 1, (4,), {"FLIPWALK_SPEC": "1", "FLIPWALK_W2": "1"}, 8192, grid(1, True)),
    # the one-chain-per-wave kernel on the same grid
    ("wave64-4x4", "g4x4", "cutedge", MU, "cut", 1, (12,), {"FLIPWALK_NO_GRID16": "1"}, N, chain(4)),
    # W = 3 (5 rows of 3): always that kernel, at 3- and 4-bit labels
    ("wave64-5x3-lb3", "g5x3", "pairs", 0.5, "cut", 2, (12,), {"FLIPWALK_CSR_LB": "3"}, N, chain(3)),
    ("wave64-5x3-lb4", "g5x3", "cutedge", MU, "cut", 1, (4,), {"FLIPWALK_CSR_LB": "4"}, N, chain(4)),
    # padded-row CSR kernel: 4-bit labels (the default at k + maxdeg = 10), 5-bit forced, and
    # the 8-bit in-place codes a hub of degree 14 needs (k + maxdeg = 16)
    ("csr-del18-lb4", "del18", "cutedge", 0.5, "cut", 2, (4,), {}, N, chain(4)),
    ("csr-del18-lb5", "del18", "pairs", MU, "cut", 1, (4,), {"FLIPWALK_CSR_LB": "5"}, N, chain(5)),
    ("csr-hub14-lb8", "hub14", "pairs", MU, "cut", 1, (2,), {"FLIPWALK_CSR_LB": "8"}, N, chain(8)),
    ("csr-hub14-lb8-cutedge", "hub14", "cutedge", 0.5, "cut", 2, (2,), {"FLIPWALK_CSR_LB": "8"}, N, chain(8)),
    # CSR-walking kernel (a hub of degree 18: no padded-row table)
    ("walk-hub5-pairs", "hub5", "pairs", MU, "cut", 1, (2,), {}, N, chain(8)),
    ("walk-hub5-cutedge", "hub5", "cutedge", 0.5, "cut", 2, (2,), {}, N, chain(8)),
    # FULL instantiation: the other accept rules
    ("full-4x4-bratio", "g4x4", "pairs", MU, "bratio", 1, (4,), {}, N, {"kernel": "grid", "bits": 2}),
    ("full-4x4-boundary", "g4x4", "cutedge", MU, "boundary", 2, (4,), {}, N, {"kernel": "grid", "bits": 2}),
    ("full-del18-bratio", "del18", "cutedge", MU, "bratio", 2, (4,), {}, N, chain(4)),
    ("full-del18-boundary", "del18", "pairs", MU, "boundary", 1, (4,), {}, N, chain(4)),
    # many units per wave, three slices per unit
    ("slices-4x4", "g4x4", "pairs", MU, "cut", 2, (12,), {"FLIPWALK_GRID_CAP": "1", "FLIPWALK_SLICES": "3"}, N, {"kernel": "grid", "bits": 2}),
    # t = 12 as three launches of 4
    ("split-4x4", "g4x4", "pairs", 0.5, "cut", 1, (4, 4, 4), {}, N, {"kernel": "grid", "bits": 2}),
]


def assert_kernel(fid, want, err, bits, maxdeg):
    """The plan lines the library printed and the handle's label width against ``want``."""
    grid_lines = [ln for ln in err.splitlines() if ln.startswith("flipwalk: grid kernel")]
    chain_lines = [ln for ln in err.splitlines() if ln.startswith("flipwalk: chain kernel")]
    assert bits == want["bits"], (fid, "label bits", bits)
    if want["kernel"] == "chain":
        assert chain_lines and not grid_lines, (fid, err)
        assert (maxdeg > 16) == fid.startswith("walk"), (fid, maxdeg)
        return
    assert grid_lines and not chain_lines, (fid, err)
    for ln in grid_lines:
        assert "small-grid plan" in ln and f"{want['bits']}-bit labels" in ln, ln
        if "rows" in want:
            assert f"{want['rows']} row(s) per chain" in ln, ln
            assert ("(W2 register budget)" in ln) == want["w2"], ln


def assert_stats_equal(gpu, orc):
    for f in orc.dtype.names:
        a, b = gpu[f], orc[f]
        if f == "sum_invb":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (f, a, b)


@pytest.mark.parametrize("fid,name,mode,base,rule,si,launches,knobs,n,want", FAMILIES,
                         ids=[f[0] for f in FAMILIES])
def test_kernels_follow_the_exact_law(gpu_lib, fid, name, mode, base, rule, si, launches, knobs,
                                      n, want, monkeypatch, capfd):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("FLIPWALK_VERBOSE", "1")
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    g, k, bounds, _, flags = LC.graph_case(name)
    x0 = LC.start_plans(name)[si]
    init = np.array(x0, np.int16)
    thr = LC.thr_table(name, base, rule)
    fl = flags if rule == "boundary" else None
    capfd.readouterr()
    dg = DeviceGraph(g)
    ch = Chains(dg, n, k, init, proposal=mode, pop_bounds=bounds, seed=SEED, chain_id0=0, thr=thr)
    if rule != "cut":
        ch.set_accept(rule, fl)
    for s in launches:
        ch.run(s)
    labels, stats = ch.labels(), ch.stats()
    bits, maxdeg = ch.overlap_info()["label_bits"], dg.maxdeg
    ch.close()
    dg.close()
    assert_kernel(fid, want, capfd.readouterr().err, bits, maxdeg)
    t = sum(launches)
    # parity first: the first and the last 64 chains against the oracle, bit for bit
    ids = list(range(64)) + list(range(n - 64, n))
    for i in ids:
        lab, st = init, O.new_stats(1)
        for s in launches:
            lab, st, _, _ = O.run_chain(g, lab, k, LC.MODE_ID[mode], *bounds, thr, SEED, i, s,
                                        stats=st, accept_rule=LC.RULE_ID[rule], flags=fl)
        assert np.array_equal(labels[i], lab), ("parity", fid, i)
        assert_stats_equal(stats[i:i + 1], st)
    LC.check_law(LC.chain_law(name, mode, base, rule), x0, t, labels, stats, f"gpu {fid}")


def test_replica_exchange_follows_the_exact_joint_law(gpu_lib, monkeypatch):
    """32,768 two-rung replica sets (bases 0.5 and MU, 4 x 4, k = 2), run_tempered(2, 2): the
    pair (plan on rung 0, plan on rung 1) against the exact joint law from the law_ref rows and
    the swap probability min(1, (b0 / b1)^(cut0 - cut1)), the pair (0, 1) tried on even rounds
    only; each rung's marginal after the exchange against the exact marginal."""
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    g, k, bounds, seed, joint = LC.tempered_case()
    dg = DeviceGraph(g)
    ch = Chains(dg, N, k, seed, proposal="pairs", pop_bounds=bounds, base=1.0, seed=SEED + 2)
    ch.set_ladder((0.5, MU))
    ch.run_tempered(2, 2)
    labels, rungs, rs = ch.labels(), ch.rungs(), ch.rung_stats()
    ch.close()
    dg.close()
    assert (rs["swap_tried"][:, 0] == 1).all() and not rs["swap_tried"][:, 1].any()
    assert 0 < rs["swap_done"].sum() < N // 2
    LC.check_tempered(joint, labels, rungs, N // 2, "gpu ladder")
