"""Per-district geometry on the GPU (fw_chains_set_geometry / fw_chains_geometry_async) against
the numpy restatement in geometry_ref.py.  Every comparison is exact (``np.array_equal``) and
is made against ``labels()`` read at the same point."""
import numpy as np
import pytest

import geometry_ref
from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, grid_graph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8", "FLIPWALK_GEOM_TILE",
            "FLIPWALK_GEOM_BINS", "FLIPWALK_GEOM_NW")
BIG = 2 ** 31 - 1


def graph_of(name):
    """(graph, seed plan, k, proposal mode, bounds, base) of a tests/cases.py case or of one of
    the two square grids test_gpu_tally.py builds, built the same way."""
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
    return Chains(DeviceGraph(g), n_chains, k, init, proposal=mode, pop_bounds=bounds, base=base,
                  seed=seed, **kw)


def random_array(rng, length):
    """Integers in 0..999, about 30% of them zero."""
    return (rng.integers(0, 1000, length) * (rng.random(length) < 0.7)).astype(np.int64)


def big_array(rng, length, at):
    """A total of exactly 2^31 - 1, almost all of it on entry ``at`` (a signed or narrow
    accumulator shows there)."""
    a = rng.integers(0, 5, length).astype(np.int64)
    a[at] = 0
    a[at] = BIG - int(a.sum())
    assert int(a.sum()) == BIG
    return a


def make_arrays(g, seed, big=None):
    """(edge weights, area, exterior) of a graph; ``big`` names the one that totals 2^31 - 1."""
    rng = np.random.default_rng(seed)
    w, a, x = random_array(rng, g.n_edges), random_array(rng, g.n), random_array(rng, g.n)
    if big == "w":
        w = big_array(rng, g.n_edges, g.n_edges // 3)
    elif big == "a":
        a = big_array(rng, g.n, g.n // 3)
    elif big == "x":
        x = big_array(rng, g.n, (2 * g.n) // 3)
    return w, a, x


def reference(ch, arrays=(None, None, None), groups=None, n_groups=1):
    """(G, one measurement's histogram) of the plans the handle holds now."""
    g = ch.dgraph.graph
    G = geometry_ref.districts(ch.labels(), g.edges(), ch.k, *arrays)
    return G, geometry_ref.cut_hist(G, g.n_edges, groups, n_groups)


def check_invariants(ch, G, arrays, ran=True):
    """``ran``: the handle has run (a stats record's cut is derived by the first launch)."""
    g = ch.dgraph.graph
    w, a, x = arrays
    if ran:
        assert np.array_equal(G[:, :, 1].sum(axis=1), 2 * ch.stats()["cut"].astype(np.int64))
    assert (G[:, :, 0].sum(axis=1) == g.n).all()
    assert (G[:, :, 3].sum(axis=1) == (0 if x is None else int(x.sum()))).all()
    assert (G[:, :, 4].sum(axis=1) == (g.n if a is None else int(a.sum()))).all()
    if w is None:
        assert np.array_equal(G[:, :, 2], G[:, :, 1])


# (case, environment, label bits expected, chains, the array that totals 2^31 - 1)
WIDTH_CASES = [
    ("grid7x9_k3_cut", {}, 2, 5, "w"),     # 63 nodes, 110 edges: less than one step, one tile
    ("grid11x13_k4", {}, 2, 77, "a"),      # ragged node and edge tails; last workgroup not full
    ("grid40x3_k2_cut", {}, 4, 1, "x"),    # W = 3: the chain kernel's record on a grid
    ("grid40_k4", {}, 2, 77, "w"),         # 3,120 edges: several edge tiles, several workgroups
    ("grid40_k4", {"FLIPWALK_NO_GRID16": "1", "FLIPWALK_CSR_LB": "3"}, 3, 5, "a"),
    ("grid16x24_k8", {}, 4, 5, "x"),       # the 8-accumulator instantiation
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5"}, 5, 5, "w"),   # LDS bins, 5-bit, irregular edges
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8, 77, "a"),  # bins with many chains
    ("hub_k3", {}, 8, 5, "x"),             # degrees 30 and 22 on the register path
    ("big132_k8", {"FLIPWALK_BIG_K8": "1"}, 3, 5, "w"),  # 6.5 KB label copies: 116 KB of LDS
    # the plan's other paths, forced on the small shapes: bins with 3, 2 and 1 quantities a
    # walk, districts 8 at a time in registers (the fallback when no bins fit), 64-entry tiles
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5", "FLIPWALK_GEOM_BINS": "3"}, 5, 5, "x"),
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5", "FLIPWALK_GEOM_BINS": "2"}, 5, 5, "a"),
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8", "FLIPWALK_GEOM_BINS": "1"}, 8, 5, "w"),
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8", "FLIPWALK_GEOM_BINS": "0"}, 8, 5, "w"),
    ("grid11x13_k4", {"FLIPWALK_GEOM_TILE": "64", "FLIPWALK_GEOM_NW": "3"}, 2, 5, "w"),
]


def case_id(c):
    forced = "".join(f"-{k[14:].lower()}{v}" for k, v in c[1].items() if k.startswith("FLIPWALK_GEOM"))
    return f"{c[0]}-lb{c[2]}-c{c[3]}-{c[4]}{forced}"


@pytest.mark.parametrize("name,env,bits,n_chains,big", WIDTH_CASES,
                         ids=[case_id(c) for c in WIDTH_CASES])
def test_geometry_matches_reference(gpu_lib, name, env, bits, n_chains, big, monkeypatch):
    """Seed plan, then 200 steps: all five columns and the histogram of both measurements."""
    ch = make(name, n_chains, env, monkeypatch)
    g = ch.dgraph.graph
    arrays = make_arrays(g, seed=len(name) + n_chains, big=big)
    ch.set_geometry(*arrays)
    info = ch.geometry_info()
    assert (info["edge_weights"], info["label_bits"], info["n_groups"], info["n_edges"],
            info["n_measured"]) == (True, bits, 1, g.n_edges, 0)
    ch.geometry()
    G, H = reference(ch, arrays)
    got = ch.district_geometry()
    assert got.dtype == np.int64 and np.array_equal(got, G)
    check_invariants(ch, got, arrays, ran=False)
    ch.run(200)
    ch.geometry()
    G, h = reference(ch, arrays)
    assert not np.array_equal(ch.labels()[0], graph_of(name)[1])  # the plans did move
    got = ch.district_geometry()
    assert np.array_equal(got, G)
    check_invariants(ch, got, arrays)
    assert np.array_equal(ch.geometry_hist(), H + h)
    assert ch.geometry_info()["n_measured"] == 2


@pytest.mark.parametrize("name,env", [
    ("grid11x13_k4", {}), ("grid16x24_k8", {}), ("delaunay3k_k18", {}),
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5", "FLIPWALK_GEOM_BINS": "2"})],
    ids=["grid11x13_k4", "grid16x24_k8", "delaunay3k_k18", "delaunay3k_k31-bins2"])
def test_unit_weights_and_population_area(gpu_lib, name, env, monkeypatch):
    """edge_weights=None: column 2 equals column 1; area = the populations: column 4 equals
    pops(); no exterior: column 3 is zero.  Then everything None: area counts the nodes."""
    ch = make(name, 5, env, monkeypatch)
    pop = ch.dgraph.graph.pop_array()
    ch.set_geometry(area=pop)
    assert ch.geometry_info()["edge_weights"] is False
    for steps in (0, 200):
        if steps:
            ch.run(steps)
        ch.geometry()
        got = ch.district_geometry()
        assert np.array_equal(got, reference(ch, (None, pop, None))[0])
        assert np.array_equal(got[:, :, 2], got[:, :, 1]) and got[:, :, 1].any()
        assert np.array_equal(got[:, :, 4], ch.pops()) and not got[:, :, 3].any()
        check_invariants(ch, got, (None, pop, None), ran=steps > 0)
    assert not np.array_equal(ch.labels()[0], graph_of(name)[1])
    ch.set_geometry()
    ch.geometry()
    got = ch.district_geometry()
    assert np.array_equal(got, reference(ch)[0])
    assert np.array_equal(got[:, :, 4], got[:, :, 0])


def test_measurements_are_ordered_on_the_stream(gpu_lib, monkeypatch):
    """run_async(100); geometry() with no sync in between equals run(100); geometry() on a
    twin handle, three times over."""
    a = make("grid11x13_k4", 77, {}, monkeypatch)
    b = make("grid11x13_k4", 77)
    arrays = make_arrays(a.dgraph.graph, seed=5)
    a.set_geometry(*arrays)
    b.set_geometry(*arrays)
    H = 0
    for _ in range(3):
        a.run_async(100)
        a.geometry()
        b.run(100)
        b.geometry()
        G, h = reference(b, arrays)
        assert np.array_equal(b.district_geometry(), G)
        H = H + h
    a.sync()
    assert not np.array_equal(b.labels()[0], graph_of("grid11x13_k4")[1])
    assert np.array_equal(a.district_geometry(), G)
    assert np.array_equal(a.geometry_hist(), H) and np.array_equal(b.geometry_hist(), H)
    assert a.geometry_info()["n_measured"] == 3


def ladder_pair(monkeypatch):
    out = []
    for _ in range(2):
        ch = make("grid12_k4_pairs", 32, {}, monkeypatch, seed=9)
        ch.set_ladder(np.geomspace(0.7, 1.4, 8))
        out.append(ch)
    return out


def test_histogram_by_rung(gpu_lib, monkeypatch):
    """8 rungs x 4 sets, run_tempered(20, 6, geometry=True): a plan is measured under the rung
    it has just run on (the measurement precedes the exchange); the reference replays the
    rounds synchronously and reads labels() and rungs() before each exchange."""
    a, b = ladder_pair(monkeypatch)
    arrays = make_arrays(a.dgraph.graph, seed=3)
    a.set_geometry(*arrays)
    assert a.geometry_info()["n_groups"] == 8
    seed_plan = a.labels()
    a.run_tempered(20, 6, geometry=True)
    H, moved = 0, False
    for i in range(6):
        b.run(20)
        rungs = b.rungs()
        moved = moved or not np.array_equal(rungs, np.arange(32) % 8)
        G, h = reference(b, arrays, rungs, 8)
        H = H + h
        b.exchange(i)
        b.sync()
    assert moved and not np.array_equal(b.labels(), seed_plan)
    got = a.geometry_hist()
    assert got.shape == (8, a.dgraph.n_edges + 1) and np.array_equal(got, H)
    assert (got.sum(axis=1) == 6 * 4 * 4).all()  # rounds x sets x districts on every rung
    assert np.array_equal(a.district_geometry(), G)
    assert a.geometry_info()["n_measured"] == 6
    # set_ladder after set_geometry re-sizes the histogram and zeroes it
    a.set_ladder(np.geomspace(0.7, 1.4, 4))
    assert a.geometry_hist().shape == (4, a.dgraph.n_edges + 1) and not a.geometry_hist().any()
    a.geometry()
    G, h = reference(a, arrays, a.rungs(), 4)
    assert np.array_equal(a.geometry_hist(), h) and np.array_equal(a.district_geometry(), G)


def test_resets_and_state(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    arrays = make_arrays(ch.dgraph.graph, seed=8)
    ch.set_geometry(*arrays)
    ch.geometry()
    ch.run(200)
    assert not np.array_equal(ch.labels()[0], graph_of("grid11x13_k4")[1])
    ch.geometry()
    hist = ch.geometry_hist()
    assert int(hist.sum()) == 2 * 5 * 4
    ch.reset_observables()  # leaves the geometry alone, as it leaves the tally alone
    assert np.array_equal(ch.geometry_hist(), hist) and ch.geometry_info()["n_measured"] == 2
    G, h = reference(ch, arrays)
    assert np.array_equal(ch.district_geometry(), G)
    ch.geometry_reset()
    assert not ch.geometry_hist().any() and ch.geometry_info()["n_measured"] == 0
    ch.geometry()
    assert np.array_equal(ch.geometry_hist(), h) and ch.geometry_info()["n_measured"] == 1
    ch.set_geometry(arrays[0][::-1].copy(), None, arrays[2])  # a second set_geometry
    assert not ch.geometry_hist().any() and ch.geometry_info()["n_measured"] == 0
    with pytest.raises(_lib.FlipwalkError) as e:  # nothing measured since the new arrays
        ch.district_geometry()
    assert e.value.code == _lib.FW_ESTATE
    ch.geometry()
    assert np.array_equal(ch.district_geometry(),
                          reference(ch, (arrays[0][::-1], None, arrays[2]))[0])


def test_errors(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L, g = _lib.load(), ch.dgraph.graph
    n, E = g.n, g.n_edges

    def code(call):
        with pytest.raises(_lib.FlipwalkError) as e:
            call()
        return e.value.code

    # before set_geometry
    assert code(ch.geometry) == _lib.FW_ESTATE
    assert code(ch.geometry_hist) == _lib.FW_ESTATE
    assert code(ch.district_geometry) == _lib.FW_ESTATE
    hist = np.zeros(E + 1, np.uint64)
    assert L.fw_chains_write_geometry(ch._h, _lib.GEOM_HIST, _lib.ptr(hist), hist.nbytes) == \
        _lib.FW_ESTATE
    assert ch.geometry_info()["n_measured"] == 0
    # the library's own checks (the Python layer refuses these before it is called)
    neg = np.ones(E, np.int64)
    neg[17] = -1
    assert L.fw_chains_set_geometry(ch._h, _lib.ptr(neg), None, None) == _lib.FW_EINVAL
    over = np.zeros(n, np.int64)
    over[3], over[140] = 2 ** 31 - 5, 5  # a total of exactly 2^31
    assert L.fw_chains_set_geometry(ch._h, None, _lib.ptr(over), None) == _lib.FW_EINVAL
    assert L.fw_chains_set_geometry(ch._h, None, None, _lib.ptr(over)) == _lib.FW_EINVAL
    assert code(ch.geometry) == _lib.FW_ESTATE  # the refused calls set nothing
    with pytest.raises(ValueError):
        ch.set_geometry(area=over)
    with pytest.raises(ValueError):
        ch.set_geometry(edge_weights=np.ones(E))  # floats
    over[140] = 4  # 2^31 - 1 is allowed
    ch.set_geometry(area=over, exterior=over)
    assert code(ch.district_geometry) == _lib.FW_ESTATE  # set, but nothing measured yet
    assert not ch.geometry_hist().any()
    ch.geometry()
    got = ch.district_geometry()
    assert (got[:, :, 3].sum(axis=1) == BIG).all() and (got[:, :, 4].sum(axis=1) == BIG).all()
    # wrong byte counts and kinds
    buf = np.zeros(5 * 4 * 5, np.int64)
    assert L.fw_chains_read_geometry(ch._h, _lib.GEOM_DISTRICTS, _lib.ptr(buf),
                                     buf.nbytes - 8) == _lib.FW_EINVAL
    assert L.fw_chains_read_geometry(ch._h, _lib.GEOM_HIST, _lib.ptr(hist),
                                     hist.nbytes - 8) == _lib.FW_EINVAL
    assert L.fw_chains_write_geometry(ch._h, _lib.GEOM_HIST, _lib.ptr(hist),
                                      hist.nbytes - 8) == _lib.FW_EINVAL
    assert L.fw_chains_write_geometry(ch._h, _lib.GEOM_DISTRICTS, _lib.ptr(buf),
                                      buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_read_geometry(ch._h, 7, _lib.ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_read_geometry(ch._h, _lib.GEOM_DISTRICTS, _lib.ptr(buf),
                                     buf.nbytes) == _lib.FW_OK
    assert np.array_equal(buf.reshape(5, 4, 5), got)


def test_checkpoint_carries_the_geometry(gpu_lib, monkeypatch, tmp_path):
    """save_checkpoint -> from_checkpoint keeps the arrays, the histogram and the count, and
    the next measurement on the restored handle equals the original's."""
    whole = make("grid11x13_k4", 5, {}, monkeypatch)
    g, _, k, _, _, _ = graph_of("grid11x13_k4")
    w, _, x = make_arrays(g, seed=2)
    whole.set_geometry(w, None, x)
    for _ in range(2):
        whole.run_async(100)
        whole.geometry()
    whole.sync()
    path = str(tmp_path / "ck.npz")
    whole.save_checkpoint(path)
    resumed = Chains.from_checkpoint(DeviceGraph(g), path, k)
    rw, ra, rx = resumed.geometry_arrays
    assert np.array_equal(rw, w) and ra is None and np.array_equal(rx, x)
    assert np.array_equal(resumed.geometry_hist(), whole.geometry_hist())
    assert resumed.geometry_info()["n_measured"] == 2
    assert resumed.geometry_info()["edge_weights"] is True
    for ch in (whole, resumed):
        ch.run_async(100)
        ch.geometry()
        ch.sync()
    assert np.array_equal(resumed.labels(), whole.labels())
    assert not np.array_equal(whole.labels()[0], graph_of("grid11x13_k4")[1])
    assert np.array_equal(resumed.district_geometry(), whole.district_geometry())
    assert np.array_equal(resumed.district_geometry(), reference(whole, (w, None, x))[0])
    assert np.array_equal(resumed.geometry_hist(), whole.geometry_hist())
    assert resumed.geometry_info()["n_measured"] == whole.geometry_info()["n_measured"] == 3


def test_tally_and_geometry_share_a_handle(gpu_lib, monkeypatch):
    """A tally and a geometry call on one handle do not disturb each other or the run:
    run_sampled(tally=True, geometry=True) ends with the plans, stats and series of a plain
    handle, one measurement per sample, and both results equal their references."""
    import tally_ref
    plain = make("grid40_k4", 77, {}, monkeypatch)
    both = make("grid40_k4", 77)
    arrays = make_arrays(both.dgraph.graph, seed=6, big="a")
    cols = np.random.default_rng(7).integers(0, 1000, (2, 1600))
    both.set_columns(cols)
    both.set_elections([(0, 1)])
    both.set_geometry(*arrays)
    for ch in (plain, both):
        ch.enable_series(4)
    plain.run_sampled(60, 4)
    both.run_sampled(60, 4, tally=True, geometry=True)
    assert both.geometry_info()["n_measured"] == 4 and both.tally_info()["n_tallied"] == 4
    assert int(both.geometry_hist().sum()) == 4 * 77 * 4
    assert np.array_equal(plain.labels(), both.labels())
    assert not np.array_equal(plain.labels()[0], graph_of("grid40_k4")[1])
    assert plain.stats().tobytes() == both.stats().tobytes()
    assert np.array_equal(plain.series("cut"), both.series("cut"))
    assert np.array_equal(plain.hist_cut(), both.hist_cut())
    assert np.array_equal(both.district_geometry(), reference(both, arrays)[0])
    T, S, _ = tally_ref.tally(both.labels(), cols, 4, [(0, 1)])
    assert np.array_equal(both.tallies(), T) and np.array_equal(both.seats(), S)
    both.geometry()
    both.tally()  # the other order
    assert np.array_equal(both.district_geometry(), reference(both, arrays)[0])
    assert np.array_equal(both.tallies(), T)
