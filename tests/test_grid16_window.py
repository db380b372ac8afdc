"""The grid kernel's 7x7 contiguity window, one window row per lane, against the CPU oracle.

The window stage (csrc/fw_window_rows.h, run by grid16_body) reads each window row as one
dword pair and masks what lies off the grid, so the cases are the grids where that masking
works hardest: grids narrower or lower than the window (every window clipped, rows wrapping
into the next grid row inside the pair), one grid per label width (2, 4 and 3 bits: the row
mask's three forms), and every kind of instantiation that shares the body (R = 1 under both
register budgets, speculative R = 2 and 4, large-grid, FULL).  Every case is bit for bit:
final plans, populations, all stats fields and both histograms equal
oracle/flipchain_oracle.c.  bfs_runs and bfs_nodes are the fields a wrong window moves: an
"undecided" where the oracle decides is an extra search, a wrong verdict another trajectory.

Each case also shows that its windows decided both ways and left some undecided: proposals
failed contiguity, exact searches ran, and fewer of them than contiguity checks that ended
in a verdict (rejections plus accepted flips).
"""
import numpy as np
import pytest

from cases import MU, Case
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph
from flipcomplexityempirical_amd.graph import band_seed, block_seed, grid_graph, stripe_seed
from oracle import oracle as O
from test_gpu_parity import CASES, _run_vs_oracle, assert_stats_equal

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in CASES}
BY_NAME["grid7_k2"] = Case("grid7_k2", grid_graph(7, 7), stripe_seed(7, 7), 2, 1, 0.30, 0.8)
BY_NAME["grid12x5_k2"] = Case("grid12x5_k2", grid_graph(12, 5), band_seed(12, 5, 2), 2, 1, 0.20, 0.8)
BY_NAME["grid9x7_k3"] = Case("grid9x7_k3", grid_graph(9, 7), band_seed(9, 7, 3), 3, 1, 0.30, MU)
# 4-bit labels: 5 <= k <= 15 on a small grid
BY_NAME["grid20x21_k6"] = Case("grid20x21_k6", grid_graph(20, 21), block_seed(20, 21, 2, 3), 6, 1,
                               0.30, 0.8)
# 3-bit labels: the large-grid plan with 5 <= k <= 8 (FLIPWALK_BIG_K8=1), the smallest grid
# of tests/test_gpu_parity.py's BIG_CASES
BY_NAME["big132_k8"] = Case("big132_k8", grid_graph(132, 132), block_seed(132, 132, 2, 4), 8, 1,
                            0.05, 0.5)

CLIPPED = ["grid7_k2", "grid9x7_k3", "grid12x5_k2", "grid3x40_k2_bi", "grid40x4_k2"]


def _env(monkeypatch, **env):
    for k in ("FLIPWALK_NO_GRID16", "FLIPWALK_SLICES", "FLIPWALK_GRID_CAP", "FLIPWALK_FOLD_AT",
              "FLIPWALK_GRID16_NW", "FLIPWALK_SPEC", "FLIPWALK_W2", "FLIPWALK_NO_BITBOARD",
              "FLIPWALK_NO_ROWBB", "FLIPWALK_BIG_K8"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FLIPWALK_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _plans(capfd):
    plans = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("flipwalk: grid kernel")]
    assert plans, "no plan line: the grid kernel did not run"
    return plans


def _window_worked(st):
    """Windows decided both ways and some stayed undecided (module docstring)."""
    fails, runs = int(st["contig_fail"].sum()), int(st["bfs_runs"].sum())
    assert fails > 0 and runs > 0, (fails, runs)
    assert runs < fails + int(st["accepts"].sum()), (runs, fails)


def _run(name, n_chains, steps_list, capfd, lb, rows, big=False, w2=None):
    capfd.readouterr()
    st = _run_vs_oracle(BY_NAME[name], n_chains, steps_list)
    for ln in _plans(capfd):
        assert ("large-grid plan" in ln) == big, ln
        assert f"{lb}-bit labels, {rows} row(s) per chain" in ln, ln
        if w2 is not None:
            assert ("(W2 register budget)" in ln) == (w2 == "1"), ln
    _window_worked(st)
    return st


@pytest.mark.parametrize("w2", ["0", "1"])
@pytest.mark.parametrize("name", CLIPPED)
def test_every_window_clipped(gpu_lib, name, w2, monkeypatch, capfd):
    """Grids of width 4, 5 and 7 and of height 3 and 7: hardly a window lies inside the grid,
    and on widths below 7 a window row's dword pair runs into the next grid row."""
    _env(monkeypatch, FLIPWALK_SPEC="1", FLIPWALK_W2=w2)
    _run(name, 45, [400, 300], capfd, 2, "1", w2=w2)


@pytest.mark.parametrize("name,lb,big,env", [
    ("grid20_k4_mu", 2, False, {}),
    ("grid20x21_k6", 4, False, {}),
    ("big132_k8", 3, True, {"FLIPWALK_BIG_K8": "1"}),
    ("big132_k8", 3, True, {"FLIPWALK_BIG_K8": "1", "FLIPWALK_NO_ROWBB": "1"}),
], ids=["lb2", "lb4", "lb3", "lb3-norow"])
def test_label_widths(gpu_lib, name, lb, big, env, monkeypatch, capfd):
    """The row mask's three forms: 2-bit labels, 4-bit (k = 6 on a width that is no multiple
    of 4) and 3-bit (the large-grid plan, with and without its 16x32 row search behind the
    window)."""
    _env(monkeypatch, FLIPWALK_SPEC="1", **env)
    _run(name, 13 if big else 37, [300, 200], capfd, lb, "1", big=big)


@pytest.mark.parametrize("rows,w2", [("1", "0"), ("1", "1"), ("2", "0"), ("4", "0")])
@pytest.mark.parametrize("name", ["grid20_k4_mu", "grid30x18_k2_bi"])
def test_lean_kernel_modes(gpu_lib, name, rows, w2, monkeypatch, capfd):
    """R = 1 under the 3-waves-per-SIMD budget and under W2, and the speculative kernels
    (R = 2, 4), where the rows of one chain run their windows on the same labels."""
    _env(monkeypatch, FLIPWALK_SPEC=rows, FLIPWALK_W2=w2)
    _run(name, 37, [400, 300], capfd, 2, rows, w2=w2 if rows == "1" else None)


@pytest.mark.parametrize("name,lb", [("grid20_k4_mu", 2), ("grid20x21_k6", 4)])
def test_full_instantiation(gpu_lib, name, lb, monkeypatch, capfd):
    """The FULL instantiation (the |B'|/|B| accept rule switches it on) runs the same window."""
    from flipcomplexityempirical_amd.chain import annealing_table
    _env(monkeypatch)
    case = BY_NAME[name]
    g = case.graph
    thr = annealing_table(0.1, 5, g.maxdeg)
    n_chains, seed, id0, steps_list = 21, 77, 40, [400, 300]
    capfd.readouterr()
    dg = DeviceGraph(g)
    ch = Chains(dg, n_chains, case.k, case.init, proposal=case.mode, pop_bounds=case.bounds,
                seed=seed, chain_id0=id0, thr=thr)
    ch.set_accept("bratio")
    for s in steps_list:
        ch.run(s)
    labs, st = ch.labels(), ch.stats()
    for ln in _plans(capfd):
        assert f"{lb}-bit labels" in ln, ln
    lo, hi = case.bounds
    hc = np.zeros(g.n_edges + 1, np.uint64)
    hb = np.zeros(g.n + 1, np.uint64)
    for i in range(n_chains):
        lab, ost = case.init.copy(), O.new_stats(1)
        for s in steps_list:
            lab, ost, _, _ = O.run_chain(g, lab, case.k, case.mode, lo, hi, thr, seed, id0 + i, s,
                                         stats=ost, accept_rule=1, hist_cut=hc, hist_b=hb)
        assert np.array_equal(labs[i], lab), (name, i)
        assert_stats_equal(st[i:i + 1], ost)
    assert np.array_equal(ch.hist_cut(), hc) and np.array_equal(ch.hist_b(), hb)
    _window_worked(st)
