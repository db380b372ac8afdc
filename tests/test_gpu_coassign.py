"""The node co-assignment step on the GPU (fw_chains_enable_coassign / fw_chains_coassign_async)
against the numpy restatement in coassign_ref.py.  Every comparison is exact (``np.array_equal``)
and is made against ``labels()`` and ``rungs()`` read at the same point.  The shapes are
test_gpu_census.py's WIDTH_CASES: every label width, 63 and 143 nodes, 1, 5 and 77 chains, the hub
graph, k = 31 and the 17,424-node 3-bit plan; small graphs list all nodes, the 3,000- and
17,424-node graphs about 200, given shuffled."""
import numpy as np
import pytest

import coassign_ref
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import coassign as scores
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph
from test_gpu_census import IDS, WIDTH_CASES, graph_of

pytestmark = pytest.mark.gpu

ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8", "FLIPWALK_COA_TILE",
            "FLIPWALK_COA_CHUNK", "FLIPWALK_COA_STAGE")


def make(name, n_chains, env=None, monkeypatch=None, seed=77, **kw):
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in (env or {}).items():
        monkeypatch.setenv(key, val)
    g, init, k, mode, bounds, base = graph_of(name)
    ch = Chains(DeviceGraph(g), n_chains, k, init, proposal=mode, pop_bounds=bounds, base=base,
                seed=seed, **kw)
    ch.graph = g
    return ch


def node_list(n, lb, size=200, seed=3):
    """About ``size`` distinct nodes, shuffled: node 0, node n - 1, two runs of consecutive
    nodes, nodes whose fields straddle dwords (3 and 5 bits), the rest spread at random."""
    rng = np.random.default_rng(seed)
    keep = {0, n - 1}
    keep.update(range(20, 60))
    keep.update(range(n // 2, n // 2 + 30))
    straddle = [x for x in range(n) if (x * lb) % 32 + lb > 32]
    keep.update(straddle[:6] + straddle[-6:])
    rest = rng.permutation(n)
    for x in rest:
        if len(keep) >= size:
            break
        keep.add(int(x))
    out = np.array(sorted(keep), np.int64)
    rng.shuffle(out)
    return out


def list_for(ch, bits):
    n = ch.dgraph.n
    return None if n <= 1000 else node_list(n, bits)


def read(ch):
    return {"together": ch.coassignment(), "cnt": ch.coassign_counts()}


def ref_now(ch, nodes):
    groups = ch.coassign_info()["n_groups"]
    return coassign_ref.coassign(ch.labels(), ch.k, nodes, ch.rungs() if ch.n_rungs else None,
                                 groups)


def assert_equal(got, want):
    for key in ("together", "cnt"):
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), key
    t, cnt = got["together"], got["cnt"]
    assert np.array_equal(t, t.transpose(0, 2, 1))
    assert np.array_equal(np.diagonal(t, axis1=1, axis2=2),
                          np.broadcast_to(cnt[:, None], t.shape[:2]))


def canonical_edges(g):
    """pairs u < w in CSR row order: the census's edge ids"""
    rowptr, col = np.asarray(g.rowptr), np.asarray(g.col)
    u = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    keep = col > u
    return u[keep], col[keep]


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_coassign_matches_reference_and_invariants(gpu_lib, name, env, bits, n_chains, monkeypatch):
    ch = make(name, n_chains, env, monkeypatch)
    n = ch.dgraph.n
    nodes = list_for(ch, bits)
    m = n if nodes is None else len(nodes)
    seed_plan = np.asarray(graph_of(name)[1], np.int64)
    ch.enable_coassignment(nodes)
    info = ch.coassign_info()
    assert (info["m"], info["label_bits"], info["n_groups"], info["n_measured"]) == (m, bits, 1, 0)
    assert np.array_equal(ch.coassign_nodes(), np.arange(n) if nodes is None else nodes)
    # 1. the seed plans: together is cnt or 0 according to the seed
    ch.coassign()
    got = read(ch)
    sp = seed_plan if nodes is None else seed_plan[nodes]
    assert np.array_equal(got["together"][0],
                          (sp[:, None] == sp[None, :]).astype(np.uint64) * np.uint64(n_chains))
    total = ref_now(ch, nodes)
    assert_equal(got, total)
    # 2. 200 steps on, twice, accumulating
    for _ in range(2):
        ch.run(200)
        ch.coassign()
        total = coassign_ref.add(total, ref_now(ch, nodes))
        got = read(ch)
        assert_equal(got, total)
    assert ch.coassign_info()["n_measured"] == 3 and int(got["cnt"][0]) == 3 * n_chains
    if nodes is not None:
        return
    # 3. with all nodes: the invariants by independent routes, one measurement after a reset
    ch.coassign_reset()
    assert ch.coassign_info()["n_measured"] == 0 and not any(a.any() for a in read(ch).values())
    ch.coassign()
    ch.enable_census(nodes=False, edges=True, boundary=False)
    ch.census()
    ch.set_geometry()
    ch.geometry()
    one, geo = read(ch), ch.district_geometry()
    eu, ew = canonical_edges(ch.graph)
    assert np.array_equal(one["cnt"][:, None] - one["together"][:, eu, ew], ch.edge_cut_counts())
    assert np.array_equal(scores.edge_cut_from_coassign(one["together"], one["cnt"],
                                                        np.stack([eu, ew], 1)), ch.edge_cut_counts())
    assert int(one["together"].sum()) == int((geo[..., 0].astype(np.int64) ** 2).sum())


def near_list(size=150, first=1000, span=500, seed=8):
    """``size`` shuffled nodes of [first, first + span): windows short enough to stage"""
    return first + np.random.default_rng(seed).permutation(span)[:size]


FORCED = [("grid11x13_k4", {}, 2, None), ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8, 150)]
# tile 16, 32 and 64 x chunk 1, 2 and the default x windows staged or read from HBM.  77 chains
# are three member words, the last with 13 members; 130 are five, the last with 2.  Neither 143
# (all nodes of the 11 x 13 grid) nor 150 is a multiple of any tile.
PLANS = [dict({"FLIPWALK_COA_TILE": t}, **({"FLIPWALK_COA_CHUNK": c} if c else {}),
              **({"FLIPWALK_COA_STAGE": "0"} if not s else {}))
         for t in ("16", "32", "64") for c in ("1", "2", None) for s in (True, False)]


@pytest.mark.parametrize("n_chains", [77, 130])
@pytest.mark.parametrize("name,env,bits,size", FORCED, ids=[f[0] for f in FORCED])
def test_forced_plans_give_the_default_plans_result(gpu_lib, name, env, bits, size, n_chains,
                                                    monkeypatch):
    ch = make(name, n_chains, env, monkeypatch)
    nodes = None if size is None else near_list(size)
    ch.run(200)
    ch.enable_coassignment(nodes)
    ch.coassign()
    want = ref_now(ch, nodes)
    default = read(ch)
    assert_equal(default, want)
    base = ch.coassign_info()
    assert base["label_bits"] == bits and base["tile"] == 64 and base["staged"]
    for plan in PLANS:
        for key, val in plan.items():
            monkeypatch.setenv(key, val)
        ch.enable_coassignment(nodes)  # the plan is made here
        info = ch.coassign_info()
        assert info["tile"] == int(plan["FLIPWALK_COA_TILE"])
        if "FLIPWALK_COA_CHUNK" in plan:  # below every default: three member words at the least
            assert info["chunk"] == int(plan["FLIPWALK_COA_CHUNK"])
        assert info["staged"] == ("FLIPWALK_COA_STAGE" not in plan)
        ch.coassign()
        assert_equal(read(ch), default)
        for key in plan:
            monkeypatch.delenv(key)


def test_refusals(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L = _lib.load()
    n = ch.dgraph.n

    def code(f, *a):
        with pytest.raises(_lib.FlipwalkError) as e:
            f(*a)
        return e.value.code

    # before enable
    assert code(ch.coassign) == _lib.FW_ESTATE
    assert code(ch.coassignment) == _lib.FW_ESTATE
    assert code(ch.coassign_counts) == _lib.FW_ESTATE
    assert code(ch.coassign_nodes) == _lib.FW_ESTATE
    info = ch.coassign_info()
    assert info["m"] == 0 and info["n_measured"] == 0
    # lists through the raw ABI
    for bad in ([3, 2, 5], [1, 1, 2], [0, n], [-1, 4]):
        a = np.array(bad, np.int32)
        assert L.fw_chains_enable_coassign(ch._h, _lib.ptr(a), a.size) == _lib.FW_EINVAL
    a = np.array([1, 2], np.int32)
    assert L.fw_chains_enable_coassign(ch._h, _lib.ptr(a), 0) == _lib.FW_EINVAL
    assert ch.coassign_info()["m"] == 0
    with pytest.raises(ValueError):
        ch.enable_coassignment([4, 9, 4])
    # short buffers, a NODES write, unknown kinds
    nodes = np.array([9, 0, 142, 77, 31])
    ch.enable_coassignment(nodes)
    ch.run(200)
    ch.coassign()
    want = ref_now(ch, nodes)
    assert_equal(read(ch), want)
    for what, size, dtype in ((_lib.COASSIGN_TOGETHER, 25, np.uint64), (_lib.COASSIGN_CNT, 1, np.uint64),
                              (_lib.COASSIGN_NODES, 5, np.int32)):
        buf = np.zeros(size, dtype)
        assert L.fw_chains_read_coassign(ch._h, what, _lib.ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
        assert L.fw_chains_write_coassign(ch._h, what, _lib.ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
        assert L.fw_chains_read_coassign(ch._h, what, _lib.ptr(buf), buf.nbytes) == _lib.FW_OK
    buf = np.zeros(5, np.int32)
    assert L.fw_chains_read_coassign(ch._h, _lib.COASSIGN_NODES, _lib.ptr(buf), buf.nbytes) == _lib.FW_OK
    assert np.array_equal(buf, np.sort(nodes))  # the handle holds the list sorted
    assert L.fw_chains_write_coassign(ch._h, _lib.COASSIGN_NODES, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    big = np.zeros(64, np.uint64)
    for what in (3, -1, 8):
        assert L.fw_chains_read_coassign(ch._h, what, _lib.ptr(big), big.nbytes) == _lib.FW_EINVAL
        assert L.fw_chains_write_coassign(ch._h, what, _lib.ptr(big), big.nbytes) == _lib.FW_EINVAL
    # reset_observables leaves the arrays alone; re-enabling zeroes them
    ch.reset_observables()
    assert_equal(read(ch), want)
    assert ch.coassign_info()["n_measured"] == 1
    ch.enable_coassignment(nodes)
    assert ch.coassign_info()["n_measured"] == 0 and not any(a.any() for a in read(ch).values())


def test_all_nodes_of_the_large_grid_are_unsupported(gpu_lib, monkeypatch):
    ch = make("big132_k8", 5, {"FLIPWALK_BIG_K8": "1"}, monkeypatch)
    assert ch.dgraph.n ** 2 > _lib.COASSIGN_MAX_ELEMS
    with pytest.raises(_lib.FlipwalkError) as e:
        ch.enable_coassignment()
    assert e.value.code == _lib.FW_EUNSUPPORTED
    assert ch.coassign_info()["m"] == 0


def test_ladder_counts_by_rung(gpu_lib, monkeypatch):
    """4 rungs x 19 sets; six rounds of run, coassign, exchange against labels() and rungs() read
    before each exchange."""
    ch = make("grid11x13_k4", 76, {}, monkeypatch, seed=9)
    nodes = np.random.default_rng(1).permutation(ch.dgraph.n)[:50]
    ch.enable_coassignment(nodes)
    ch.coassign()  # counted without a ladder: set_ladder zeroes it
    ch.set_ladder(np.geomspace(0.7, 1.4, 4))
    info = ch.coassign_info()
    assert (info["n_groups"], info["n_measured"], info["m"]) == (4, 0, 50)
    assert not any(a.any() for a in read(ch).values())
    total, moved = None, False
    for i in range(6):
        ch.run(50)
        ch.coassign()
        rungs = ch.rungs()
        moved = moved or not np.array_equal(rungs, np.arange(76) % 4)
        total = coassign_ref.add(total, coassign_ref.coassign(ch.labels(), ch.k, nodes, rungs, 4))
        ch.exchange(i)
        ch.sync()
    assert moved
    got = read(ch)
    assert got["together"].shape == (4, 50, 50)
    assert_equal(got, total)
    assert (got["cnt"] == 19 * 6).all()
    assert not np.array_equal(got["together"][0], got["together"][3])
    # one call of run_tempered bumps the count by its rounds, and counts under the rungs
    ch.run_tempered(20, 3, coassign=True)
    assert ch.coassign_info()["n_measured"] == 9 and (ch.coassign_counts() == 19 * 9).all()
    # forced plans see the same rungs
    for plan in ({"FLIPWALK_COA_TILE": "16", "FLIPWALK_COA_CHUNK": "1"}, {"FLIPWALK_COA_STAGE": "0"}):
        for key, val in plan.items():
            monkeypatch.setenv(key, val)
        ch.enable_coassignment(nodes)
        ch.coassign()
        assert_equal(read(ch), ref_now(ch, nodes))
        for key in plan:
            monkeypatch.delenv(key)
    # set_ladder again re-sizes and zeroes; the list and the caller's order stay
    ch.set_ladder(np.geomspace(0.7, 1.4, 2))
    assert ch.coassignment().shape == (2, 50, 50)
    assert not any(a.any() for a in read(ch).values()) and ch.coassign_info()["n_measured"] == 0
    assert np.array_equal(ch.coassign_nodes(), nodes)
    ch.coassign()
    assert_equal(read(ch), ref_now(ch, nodes))
    assert (ch.coassign_counts() == 38).all()


def test_checkpoint_carries_the_coassignment(gpu_lib, monkeypatch, tmp_path):
    whole = make("grid11x13_k4", 9, {}, monkeypatch, seed=4)
    nodes = np.random.default_rng(2).permutation(whole.dgraph.n)[:40]
    whole.enable_coassignment(nodes)
    for _ in range(2):
        whole.run(100)
        whole.coassign()
    path = str(tmp_path / "ck.npz")
    whole.save_checkpoint(path)
    resumed = Chains.from_checkpoint(whole.dgraph, path, whole.k)
    resumed.graph = whole.graph
    assert resumed.coassign_info() == whole.coassign_info()
    assert np.array_equal(resumed.coassign_nodes(), nodes)
    assert_equal(read(resumed), read(whole))
    for ch in (whole, resumed):
        ch.run(100)
        ch.coassign()
    assert_equal(read(resumed), read(whole))
    assert resumed.coassign_info()["n_measured"] == whole.coassign_info()["n_measured"] == 3
    assert int(resumed.coassign_counts()[0]) == 27
    assert np.array_equal(resumed.labels(), whole.labels())


def test_coassign_leaves_the_plans_alone(gpu_lib, monkeypatch):
    """labels(), stats() and a following run are bit-identical with and without measurements in
    between (two handles, one seed); run_sampled(coassign=True) counts once per sample."""
    with_c = make("grid11x13_k4", 77, {}, monkeypatch)
    plain = make("grid11x13_k4", 77, {}, monkeypatch)
    with_c.enable_coassignment()
    for ch in (with_c, plain):
        ch.enable_series(8)
    with_c.coassign()
    with_c.run_sampled(60, 4, coassign=True)
    plain.run_sampled(60, 4)
    assert with_c.coassign_info()["n_measured"] == 5
    assert int(with_c.coassign_counts()[0]) == 5 * 77
    assert np.array_equal(with_c.labels(), plain.labels())
    assert with_c.stats().tobytes() == plain.stats().tobytes()
    assert np.array_equal(with_c.series("cut"), plain.series("cut"))
    with_c.coassign()
    for ch in (with_c, plain):
        ch.run(100)
    assert np.array_equal(with_c.labels(), plain.labels())
    assert with_c.stats().tobytes() == plain.stats().tobytes()
