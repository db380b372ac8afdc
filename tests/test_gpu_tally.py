"""District tallies of node columns and seat counts on the GPU (fw_chains_set_columns /
fw_chains_tally_async) against the numpy restatement in tally_ref.py.  Every comparison is
exact (``np.array_equal``) and is made against ``labels()`` read at the same point."""
import numpy as np
import pytest

import tally_ref
from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, grid_graph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8")
BIG = 2 ** 31 - 1


def graph_of(name):
    """(graph, seed plan, k, proposal mode, bounds, base) of a tests/cases.py case or of one of
    the two square grids this file adds."""
    if name in ("grid40_k4", "big132_k8"):
        side, blocks, k = (40, (2, 2), 4) if name == "grid40_k4" else (132, (2, 4), 8)
        g = grid_graph(side, side)
        return g, block_seed(side, side, *blocks), k, 1, population_bounds(g.total_pop, k, 0.05), 0.5
    c = CASES[name]
    return c.graph, c.init, c.k, c.mode, c.bounds, c.base


def make(name, n_chains, env=None, monkeypatch=None, seed=77, **kw):
    if monkeypatch is not None:
        for key in ENV_KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in (env or {}).items():
            monkeypatch.setenv(key, val)
    g, init, k, mode, bounds, base = graph_of(name)
    ch = Chains(DeviceGraph(g), n_chains, k, init, proposal=mode, pop_bounds=bounds, base=base,
                seed=seed, **kw)
    return ch


def make_columns(n, n_cols, seed=0):
    """Random integers with zeros; with three or more columns, column 1 is all zero; with two
    or more, the last column's total is exactly 2^31 - 1, put mostly on one node (a signed or
    narrow accumulator shows there)."""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 1000, (n_cols, n)) * (rng.random((n_cols, n)) < 0.7)
    if n_cols >= 3:
        cols[1] = 0
    if n_cols >= 2:
        big = rng.integers(0, 5, n)
        big[n // 3] = 0
        big[n // 3] = BIG - int(big.sum())
        cols[-1] = big
        assert int(cols[-1].sum()) == BIG
    return cols.astype(np.int64)


def check_last_tally(ch, cols, elections=()):
    """The last tally against the reference on the plans the handle holds now."""
    T, S, H = tally_ref.tally(ch.labels(), cols, ch.k, elections)
    assert np.array_equal(ch.tallies(), T)
    assert np.array_equal(ch.seats(), S)
    return H


# (case, environment, label bits expected, chains, columns)
WIDTH_CASES = [
    ("grid7x9_k3_cut", {}, 2, 5, 1),       # 63 nodes: less than one 64-node step
    ("grid11x13_k4", {}, 2, 77, 3),        # 143 nodes: a ragged tail; chains fill no workgroup
    ("grid40x3_k2_cut", {}, 4, 1, 2),      # W = 3: the chain kernel on a grid
    ("grid40_k4", {}, 2, 77, 8),           # 1,600 nodes: more than one staged tile
    ("grid40_k4", {"FLIPWALK_NO_GRID16": "1", "FLIPWALK_CSR_LB": "3"}, 3, 5, 2),
    ("grid16x24_k8", {}, 4, 5, 3),         # 5 <= k <= 8: eight register accumulators a column
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5"}, 5, 5, 3),   # LDS bins, fields across dwords
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8, 77, 2),
    ("hub_k3", {}, 8, 5, 8),               # 8-bit labels on the register path
    ("big132_k8", {"FLIPWALK_BIG_K8": "1"}, 3, 5, 2),  # 17,424 nodes, 3-bit grid-kernel plans
]


@pytest.mark.parametrize("name,env,bits,n_chains,n_cols", WIDTH_CASES,
                         ids=[f"{c[0]}-lb{c[2]}-c{c[3]}-j{c[4]}" for c in WIDTH_CASES])
def test_tally_matches_reference(gpu_lib, name, env, bits, n_chains, n_cols, monkeypatch):
    """Seed plan, then 200 steps: sums, {wins, ties} and the histogram of both tallies."""
    ch = make(name, n_chains, env, monkeypatch)
    cols = make_columns(ch.dgraph.n, n_cols, seed=n_cols)
    elections = [(0, n_cols - 1), (n_cols - 1, 0)] if n_cols >= 2 else []
    ch.set_columns(cols)
    ch.set_elections(elections)
    info = ch.tally_info()
    assert (info["n_cols"], info["n_elections"], info["label_bits"], info["n_groups"]) == \
        (n_cols, len(elections), bits, 1)
    ch.tally()
    H = check_last_tally(ch, cols, elections)
    ch.run(200)
    ch.tally()
    H = H + check_last_tally(ch, cols, elections)
    assert not np.array_equal(ch.labels()[0], graph_of(name)[1])  # the plans did move
    assert np.array_equal(ch.seat_hist(), H)
    assert ch.tally_info()["n_tallied"] == 2
    # every column's district sums add up to its total, the 2^31 - 1 column included
    assert np.array_equal(ch.tallies().sum(axis=2), np.tile(cols.sum(axis=1), (n_chains, 1)))


@pytest.mark.parametrize("name", ["delaunay3k_k18", "grid11x13_k4"])
def test_population_column_reproduces_pops(gpu_lib, name, monkeypatch):
    ch = make(name, 5, {}, monkeypatch)
    ch.set_columns({"TOTPOP": ch.dgraph.graph.pop_array()})
    assert ch.column_names == ["TOTPOP"]
    ch.run(200)
    ch.tally()
    assert np.array_equal(ch.tallies()[:, 0, :], ch.pops())


def test_seats_and_ties_on_the_seed_plan(gpu_lib, monkeypatch):
    """The 12 x 12 grid's four 6 x 6 blocks with votes built by hand: district 0 ties, district
    1 goes to A by a single vote, district 2 holds no votes (0 = 0, a tie), district 3 goes to
    B.  No run before the first tally."""
    ch = make("grid12_k4_pairs", 5, {}, monkeypatch)
    init = graph_of("grid12_k4_pairs")[1]
    a, b = np.zeros(144, np.int64), np.zeros(144, np.int64)
    first = [int(np.flatnonzero(init == d)[0]) for d in range(4)]
    last = [int(np.flatnonzero(init == d)[-1]) for d in range(4)]
    a[first[0]], b[last[0]] = 40, 40
    a[first[1]], b[last[1]], b[first[1]] = 21, 15, 5
    a[first[3]], b[last[3]] = 7, 9
    ch.set_columns({"pink": a, "purple": b})
    ch.set_elections([("pink", "purple"), ("purple", "pink")])
    ch.tally()
    assert ch.tallies()[2].tolist() == [[40, 21, 0, 7], [40, 20, 0, 9]]
    assert ch.seats()[2].tolist() == [[1, 2], [1, 2]]
    hist = ch.seat_hist()
    assert hist.shape == (1, 2, 5) and hist[0].tolist() == [[0, 5, 0, 0, 0]] * 2
    cols = np.stack([a, b])
    H = check_last_tally(ch, cols, [(0, 1), (1, 0)])
    ch.run(200)
    ch.tally()
    H = H + check_last_tally(ch, cols, [(0, 1), (1, 0)])
    assert np.array_equal(ch.seat_hist(), H)


def test_tallies_are_ordered_on_the_stream(gpu_lib, monkeypatch):
    """3 x (run_async(50), tally()) and one sync: the histogram is the sum of three reference
    tallies of a second, synchronously stepped handle, the sums are the last of them."""
    a = make("grid11x13_k4", 77, {}, monkeypatch)
    b = make("grid11x13_k4", 77)
    cols = make_columns(a.dgraph.n, 3, seed=5)
    elections = [(0, 2), (0, 1)]
    a.set_columns(cols)
    a.set_elections(elections)
    for _ in range(3):
        a.run_async(50)
        a.tally()
    a.sync()
    H = 0
    for _ in range(3):
        b.run(50)
        T, S, h = tally_ref.tally(b.labels(), cols, b.k, elections)
        H = H + h
    assert np.array_equal(a.seat_hist(), H)
    assert np.array_equal(a.tallies(), T) and np.array_equal(a.seats(), S)
    assert a.tally_info()["n_tallied"] == 3


def ladder_pair(monkeypatch):
    out = []
    for _ in range(2):
        ch = make("grid12_k4_pairs", 32, {}, monkeypatch, seed=9)
        ch.set_ladder(np.geomspace(0.7, 1.4, 8))
        out.append(ch)
    return out


def test_seat_histogram_by_rung(gpu_lib, monkeypatch):
    """8 rungs x 4 sets, run_tempered(20, 6, tally=True): a plan is counted under the rung it
    has just run on (the tally precedes the exchange); the reference replays the rounds
    synchronously and reads labels() and rungs() before each exchange."""
    a, b = ladder_pair(monkeypatch)
    cols = make_columns(144, 2, seed=3)
    cols[1] = np.random.default_rng(4).integers(0, 1000, 144)  # close races: seats vary
    for ch in (a, b):
        ch.set_columns(cols)
        ch.set_elections([(0, 1)])
    assert a.tally_info()["n_groups"] == 8
    a.run_tempered(20, 6, tally=True)
    H, moved = 0, False
    for i in range(6):
        b.run(20)
        rungs = b.rungs()
        moved = moved or not np.array_equal(rungs, np.arange(32) % 8)
        H = H + tally_ref.tally(b.labels(), cols, 4, [(0, 1)], rungs, 8)[2]
        b.exchange(i)
        b.sync()
    assert moved  # some chain was tallied away from its first rung
    got = a.seat_hist()
    assert got.shape == (8, 1, 5) and np.array_equal(got, H)
    assert int(got.sum()) == 6 * 32 and (got.sum(axis=(1, 2)) == 6 * 4).all()
    a.set_ladder(np.geomspace(0.7, 1.4, 4))
    assert a.seat_hist().shape == (4, 1, 5) and not a.seat_hist().any()


def test_resets_and_state(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    cols = make_columns(143, 2, seed=8)
    ch.set_columns(cols)
    ch.set_elections([(0, 1)])
    ch.run(100)
    ch.tally()
    hist = ch.seat_hist()
    assert int(hist.sum()) == 5
    ch.reset_observables()  # leaves the tally alone, as it leaves the series alone
    assert np.array_equal(ch.seat_hist(), hist) and ch.tally_info()["n_tallied"] == 1
    check_last_tally(ch, cols, [(0, 1)])
    ch.tally_reset()
    assert not ch.seat_hist().any() and ch.tally_info()["n_tallied"] == 0
    ch.tally()
    assert np.array_equal(ch.seat_hist(), hist)
    ch.set_columns(cols[::-1].copy())  # a second set_columns drops the elections
    info = ch.tally_info()
    assert (info["n_cols"], info["n_elections"]) == (2, 0)
    assert ch.seat_hist().shape == (1, 0, 5)
    with pytest.raises(_lib.FlipwalkError) as e:  # nothing tallied since the new columns
        ch.tallies()
    assert e.value.code == _lib.FW_ESTATE
    ch.tally()
    assert ch.seats().shape == (5, 0, 2)
    assert np.array_equal(ch.tallies(), tally_ref.sums(ch.labels(), cols[::-1], 4))


def test_errors(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L, n = _lib.load(), 143

    def code(call):
        with pytest.raises(_lib.FlipwalkError) as e:
            call()
        return e.value.code

    # before any columns
    assert code(ch.tally) == _lib.FW_ESTATE
    assert code(ch.seat_hist) == _lib.FW_ESTATE
    assert code(lambda: ch.set_elections([(0, 1)])) == _lib.FW_ESTATE
    buf = np.zeros(5 * 8 * 4, np.int64)
    assert L.fw_chains_read_tally(ch._h, _lib.TALLY_SUMS, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_ESTATE
    ok = np.ones((2, n), np.int64)
    for n_cols in (0, 9):
        wide = np.ones((max(n_cols, 1), n), np.int64)
        assert L.fw_chains_set_columns(ch._h, _lib.ptr(wide), n_cols) == _lib.FW_EINVAL
    neg = ok.copy()
    neg[1, 17] = -1
    assert code(lambda: ch.set_columns(neg)) == _lib.FW_EINVAL
    over = np.zeros((2, n), np.int64)
    over[0, 3], over[0, 140] = 2 ** 31 - 5, 5  # a total of exactly 2^31
    assert code(lambda: ch.set_columns(over)) == _lib.FW_EINVAL
    over[0, 140] = 4  # 2^31 - 1 is allowed
    ch.set_columns(over)
    assert ch.tally_info()["n_cols"] == 2
    assert code(ch.tallies) == _lib.FW_ESTATE  # columns, but no tally yet
    assert code(lambda: ch.set_elections([(0, 2)])) == _lib.FW_EINVAL
    assert code(lambda: ch.set_elections([(-1, 0)])) == _lib.FW_EINVAL
    assert code(lambda: ch.set_elections([(1, 1)])) == _lib.FW_EINVAL
    assert code(lambda: ch.set_elections([(0, 1)] * 5)) == _lib.FW_EINVAL
    assert ch.tally_info()["n_elections"] == 0  # the refused calls changed nothing
    with pytest.raises(ValueError):
        ch.set_elections([("pink", 0)])  # no names were given
    with pytest.raises(ValueError):
        ch.set_columns(np.ones((2, n)))  # floats
    hist = np.zeros(5, np.uint64)
    assert L.fw_chains_write_tally(ch._h, _lib.TALLY_SUMS, _lib.ptr(hist), hist.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_read_tally(ch._h, 7, _lib.ptr(hist), hist.nbytes) == _lib.FW_EINVAL


def test_checkpoint_carries_the_tally(gpu_lib, monkeypatch, tmp_path):
    """save_checkpoint -> from_checkpoint -> continue gives the histogram, the count and the
    sums of the uninterrupted run; names and elections travel with it."""
    cols = {"pink": np.random.default_rng(1).integers(0, 50, 143),
            "purple": np.random.default_rng(2).integers(0, 50, 143)}
    whole = make("grid11x13_k4", 5, {}, monkeypatch)
    part = make("grid11x13_k4", 5)
    for ch in (whole, part):
        ch.set_columns(cols)
        ch.set_elections([("pink", "purple")])
    for ch, rounds in ((whole, 5), (part, 2)):
        for _ in range(rounds):
            ch.run_async(40)
            ch.tally()
        ch.sync()
    path = str(tmp_path / "ck.npz")
    part.save_checkpoint(path)
    g, _, k, mode, bounds, _ = graph_of("grid11x13_k4")
    resumed = Chains.from_checkpoint(DeviceGraph(g), path, k)
    assert resumed.column_names == ["pink", "purple"]
    assert resumed.elections.tolist() == [[0, 1]]
    assert np.array_equal(resumed.seat_hist(), part.seat_hist())
    assert resumed.tally_info()["n_tallied"] == 2
    for _ in range(3):
        resumed.run_async(40)
        resumed.tally()
    resumed.sync()
    assert np.array_equal(resumed.labels(), whole.labels())
    assert np.array_equal(resumed.seat_hist(), whole.seat_hist())
    assert np.array_equal(resumed.tallies(), whole.tallies())
    assert resumed.tally_info()["n_tallied"] == whole.tally_info()["n_tallied"] == 5


def test_run_sampled_with_tally_and_no_interference(gpu_lib, monkeypatch):
    """A handle with columns set and a tally after every launch ends with the same stats and
    plans as one without (the run kernels saw nothing), and run_sampled(tally=True) counts one
    tally per sample."""
    plain = make("grid40_k4", 77, {}, monkeypatch)
    tallied = make("grid40_k4", 77)
    cols = make_columns(1600, 3, seed=6)
    tallied.set_columns(cols)
    tallied.set_elections([(0, 1)])
    for ch in (plain, tallied):
        ch.enable_series(4)
    plain.run_sampled(60, 4)
    tallied.run_sampled(60, 4, tally=True)
    assert tallied.tally_info()["n_tallied"] == 4
    assert int(tallied.seat_hist().sum()) == 4 * 77
    assert np.array_equal(plain.labels(), tallied.labels())
    assert plain.stats().tobytes() == tallied.stats().tobytes()
    assert np.array_equal(plain.series("cut"), tallied.series("cut"))
    assert np.array_equal(plain.hist_cut(), tallied.hist_cut())
    check_last_tally(tallied, cols, [(0, 1)])
