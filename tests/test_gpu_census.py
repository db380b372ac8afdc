"""The ensemble census on the GPU (fw_chains_enable_census / fw_chains_census_async) against the
numpy restatement in census_ref.py.  Every comparison is exact (``np.array_equal``) and is made
against ``labels()`` and ``rungs()`` read at the same point.  The shapes are test_gpu_overlap.py's
WIDTH_CASES, built the same way: every label width, 63 and 143 nodes, ragged tails, 1, 5 and 77
chains, the hub graph, k = 31 and the 17,424-node 3-bit plan."""
import numpy as np
import pytest

import census_ref
from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, grid_graph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8", "FLIPWALK_CENSUS_TILE",
            "FLIPWALK_CENSUS_SLICE", "FLIPWALK_CENSUS_STAGE")

# (case, environment, label bits expected, chains): test_gpu_overlap.py's WIDTH_CASES
WIDTH_CASES = [
    ("grid7x9_k3_cut", {}, 2, 5),
    ("grid11x13_k4", {}, 2, 77),
    ("grid40x3_k2_cut", {}, 4, 1),
    ("grid40_k4", {}, 2, 77),
    ("grid40_k4", {"FLIPWALK_NO_GRID16": "1", "FLIPWALK_CSR_LB": "3"}, 3, 5),
    ("grid16x24_k8", {}, 4, 5),
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5"}, 5, 5),
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8, 77),
    ("hub_k3", {}, 8, 5),
    ("big132_k8", {"FLIPWALK_BIG_K8": "1"}, 3, 5),
]
IDS = [f"{c[0]}-lb{c[2]}-c{c[3]}" for c in WIDTH_CASES]
KEYS = ("cnt", "occ", "ecut", "bnd")


def graph_of(name):
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
    ch.graph = g
    return ch


def read(ch):
    """The four arrays the handle holds (a part that is not enabled is left out)."""
    info = ch.census_info()
    out = {"cnt": ch.census_counts()}
    if info["nodes"]:
        out["occ"] = ch.node_occupancy()
    if info["edges"]:
        out["ecut"] = ch.edge_cut_counts()
    if info["boundary"]:
        out["bnd"] = ch.boundary_counts()
    return out


def ref_now(ch):
    """The reference's census of the plans (and rungs) the handle holds now."""
    groups = ch.census_info()["n_groups"]
    return census_ref.census(ch.graph, ch.labels(), ch.k, ch.rungs() if ch.n_rungs else None,
                             groups)


def assert_equal(got, want, keys=KEYS):
    for key in keys:
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_census_matches_reference_and_invariants(gpu_lib, name, env, bits, n_chains, monkeypatch):
    ch = make(name, n_chains, env, monkeypatch)
    n, k, E = ch.dgraph.n, ch.k, ch.dgraph.n_edges
    seed_plan = np.asarray(graph_of(name)[1], np.int64)
    ch.enable_census()
    assert ch.census_info() == {"nodes": True, "edges": True, "boundary": True,
                                "label_bits": bits, "n_groups": 1, "n_edges": E, "n_measured": 0}
    # 1. the seed plans: every chain on the seed label
    ch.census()
    total = ref_now(ch)
    got = read(ch)
    onehot = np.zeros((1, n, k), np.uint64)
    onehot[0, np.arange(n), seed_plan] = n_chains
    assert np.array_equal(got["occ"], onehot)
    assert_equal(got, total)
    # 2. 200 steps on, twice
    for _ in range(2):
        ch.run(200)
        ch.census()
        total = census_ref.add(total, ref_now(ch))
        got = read(ch)
        assert_equal(got, total)
        assert np.array_equal(got["occ"].sum(axis=2), np.broadcast_to(got["cnt"][:, None], (1, n)))
    assert ch.census_info()["n_measured"] == 3
    assert int(got["cnt"][0]) == 3 * n_chains
    assert not np.array_equal(got["occ"], 3 * onehot)  # the chains have moved
    # 3. the invariants, by independent routes: one census after a reset against the geometry
    # and the stats of the same plans
    ch.census_reset()
    assert ch.census_info()["n_measured"] == 0 and not any(a.any() for a in read(ch).values())
    ch.census()
    ch.set_geometry()
    ch.geometry()
    one, geo, st = read(ch), ch.district_geometry(), ch.stats()
    assert np.array_equal(one["occ"][0].sum(axis=0).astype(np.int64), geo[..., 0].sum(axis=0))
    assert 2 * int(one["ecut"].sum()) == int(geo[..., 1].sum())
    assert int(one["ecut"].sum()) == int(st["cut"].sum())
    # stats' bnodes counts the nodes with a neighbour in another district under every proposal
    # mode: the oracle's derive() counts the nodes of weight > 0, and both weights (distinct
    # foreign labels; foreign neighbours under the cut-edge proposal) are positive exactly then
    assert int(one["bnd"].sum()) == int(st["bnodes"].sum())


FORCED = [("grid11x13_k4", {}, 2), ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8)]
# tile 64 and 100 (divides neither 143 nor 3,000: a ragged last tile, lanes without a node);
# slices of 1, 5 (77 = 15 x 5 + 2: a partly filled last slice) and 64; the counters are 32 bits
# wide, so no slice length is a narrow-counter bound: the longest slice, all 77 chains, is the
# default plan's.  STAGE 0 takes the labels from HBM instead of LDS.
PLANS = [{"FLIPWALK_CENSUS_TILE": "64", "FLIPWALK_CENSUS_SLICE": "1"},
         {"FLIPWALK_CENSUS_TILE": "100", "FLIPWALK_CENSUS_SLICE": "5"},
         {"FLIPWALK_CENSUS_TILE": "64", "FLIPWALK_CENSUS_SLICE": "64"},
         {"FLIPWALK_CENSUS_TILE": "100", "FLIPWALK_CENSUS_SLICE": "5", "FLIPWALK_CENSUS_STAGE": "0"},
         {"FLIPWALK_CENSUS_TILE": "7", "FLIPWALK_CENSUS_SLICE": "77"}]


@pytest.mark.parametrize("name,env,bits", FORCED, ids=[f[0] for f in FORCED])
def test_forced_plans_give_the_default_plans_result(gpu_lib, name, env, bits, monkeypatch):
    ch = make(name, 77, env, monkeypatch)
    ch.run(200)
    ch.enable_census()
    ch.census()
    want = ref_now(ch)
    assert_equal(read(ch), want)
    assert ch.census_info()["label_bits"] == bits
    for plan in PLANS:
        for key, val in plan.items():
            monkeypatch.setenv(key, val)
        ch.enable_census()  # the plan is made here
        ch.census()
        assert_equal(read(ch), want)
        for key in plan:
            monkeypatch.delenv(key)


def test_parts_and_refusals(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L = _lib.load()
    n, k, E = ch.dgraph.n, ch.k, ch.dgraph.n_edges

    def code(f, *a):
        with pytest.raises(_lib.FlipwalkError) as e:
            f(*a)
        return e.value.code

    assert code(ch.census) == _lib.FW_ESTATE
    assert code(ch.census_counts) == _lib.FW_ESTATE
    assert ch.census_info()["n_measured"] == 0 and not ch.census_info()["nodes"]
    for bad in (0, 8, -1):
        assert L.fw_chains_enable_census(ch._h, bad) == _lib.FW_EINVAL
    with pytest.raises(ValueError):
        ch.enable_census(False, False, False)
    ch.run(200)
    want = ref_now(ch)
    readers = {"occ": ch.node_occupancy, "ecut": ch.edge_cut_counts, "bnd": ch.boundary_counts}
    for part, kw in (("occ", "nodes"), ("ecut", "edges"), ("bnd", "boundary")):
        ch.enable_census(**{x: x == kw for x in ("nodes", "edges", "boundary")})
        assert [ch.census_info()[x] for x in ("nodes", "edges", "boundary")] == \
            [x == kw for x in ("nodes", "edges", "boundary")]
        ch.census()
        assert_equal(read(ch), want, ("cnt", part))
        for other, f in readers.items():
            if other != part:
                assert code(f) == _lib.FW_ESTATE
    # short buffers and unknown kinds
    ch.enable_census()
    ch.census()
    for what, size in ((_lib.CENSUS_OCC, n * k), (_lib.CENSUS_ECUT, E), (_lib.CENSUS_BND, n),
                       (_lib.CENSUS_CNT, 1)):
        buf = np.zeros(size, np.uint64)
        assert L.fw_chains_read_census(ch._h, what, _lib.ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
        assert L.fw_chains_write_census(ch._h, what, _lib.ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
        assert L.fw_chains_read_census(ch._h, what, _lib.ptr(buf), buf.nbytes) == _lib.FW_OK
    buf = np.zeros(n * k, np.uint64)
    assert L.fw_chains_read_census(ch._h, 3, _lib.ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    # reset_observables leaves the census alone; re-enabling zeroes
    ch.reset_observables()
    assert_equal(read(ch), want)
    assert ch.census_info()["n_measured"] == 1
    ch.enable_census()
    assert ch.census_info()["n_measured"] == 0 and not any(a.any() for a in read(ch).values())


def test_ladder_counts_by_rung(gpu_lib, monkeypatch):
    """4 rungs x 19 sets; six rounds of run, census, exchange against labels() and rungs() read
    before each exchange."""
    ch = make("grid11x13_k4", 76, {}, monkeypatch, seed=9)
    ch.enable_census()
    ch.census()  # counted without a ladder: set_ladder zeroes it
    ch.set_ladder(np.geomspace(0.7, 1.4, 4))
    info = ch.census_info()
    assert (info["n_groups"], info["n_measured"]) == (4, 0)
    assert not any(a.any() for a in read(ch).values())
    total, moved = None, False
    for i in range(6):
        ch.run(50)
        ch.census()
        rungs = ch.rungs()
        moved = moved or not np.array_equal(rungs, np.arange(76) % 4)
        total = census_ref.add(total, census_ref.census(ch.graph, ch.labels(), ch.k, rungs, 4))
        ch.exchange(i)
        ch.sync()
    assert moved
    got = read(ch)
    assert got["occ"].shape == (4, ch.dgraph.n, ch.k)
    assert_equal(got, total)
    assert (got["cnt"] == 19 * 6).all()
    assert not np.array_equal(got["ecut"][0], got["ecut"][3])
    # one call of run_tempered bumps the count by its rounds, and counts under the rungs
    ch.run_tempered(20, 3, census=True)
    assert ch.census_info()["n_measured"] == 9 and (ch.census_counts() == 19 * 9).all()
    # several slices per rung, and the labels from HBM, see the same rungs
    for plan in ({"FLIPWALK_CENSUS_SLICE": "5", "FLIPWALK_CENSUS_TILE": "100"},
                 {"FLIPWALK_CENSUS_SLICE": "19", "FLIPWALK_CENSUS_STAGE": "0"}):
        for key, val in plan.items():
            monkeypatch.setenv(key, val)
        ch.enable_census()
        ch.census()
        assert_equal(read(ch), ref_now(ch))
        for key in plan:
            monkeypatch.delenv(key)
    # set_ladder again re-sizes and zeroes
    ch.set_ladder(np.geomspace(0.7, 1.4, 2))
    assert ch.node_occupancy().shape == (2, ch.dgraph.n, ch.k)
    assert not any(a.any() for a in read(ch).values()) and ch.census_info()["n_measured"] == 0
    ch.census()
    assert_equal(read(ch), ref_now(ch))
    assert (ch.census_counts() == 38).all()


def test_checkpoint_carries_the_census(gpu_lib, monkeypatch, tmp_path):
    whole = make("grid11x13_k4", 9, {}, monkeypatch, seed=4)
    whole.enable_census(edges=False)
    for _ in range(2):
        whole.run(100)
        whole.census()
    path = str(tmp_path / "ck.npz")
    whole.save_checkpoint(path)
    resumed = Chains.from_checkpoint(whole.dgraph, path, whole.k)
    resumed.graph = whole.graph
    assert resumed.census_info() == whole.census_info()
    assert_equal(read(resumed), read(whole), ("cnt", "occ", "bnd"))
    for ch in (whole, resumed):
        ch.run(100)
        ch.census()
    assert_equal(read(resumed), read(whole), ("cnt", "occ", "bnd"))
    assert resumed.census_info()["n_measured"] == whole.census_info()["n_measured"] == 3
    assert int(resumed.census_counts()[0]) == 27
    assert np.array_equal(resumed.labels(), whole.labels())


def test_census_leaves_the_plans_alone(gpu_lib, monkeypatch):
    """labels(), stats() and a following run are bit-identical with and without censuses in
    between (two handles, one seed); run_sampled(census=True) counts once per sample."""
    with_c = make("grid11x13_k4", 77, {}, monkeypatch)
    plain = make("grid11x13_k4", 77, {}, monkeypatch)
    with_c.enable_census()
    for ch in (with_c, plain):
        ch.enable_series(8)
    with_c.census()
    with_c.run_sampled(60, 4, census=True)
    plain.run_sampled(60, 4)
    assert with_c.census_info()["n_measured"] == 5
    assert np.array_equal(with_c.labels(), plain.labels())
    assert with_c.stats().tobytes() == plain.stats().tobytes()
    assert np.array_equal(with_c.series("cut"), plain.series("cut"))
    with_c.census()
    for ch in (with_c, plain):
        ch.run(100)
    assert np.array_equal(with_c.labels(), plain.labels())
    assert with_c.stats().tobytes() == plain.stats().tobytes()
