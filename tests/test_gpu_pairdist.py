"""Pairwise plan distances on the GPU (fw_chains_pairdist_async) against the numpy restatement
in pairdist_ref.py.  Every comparison is exact (``np.array_equal``) and is made against
``labels()`` read at the same point.  The shapes are test_gpu_overlap.py's WIDTH_CASES, built
the same way: 63 nodes (two groups, a partial last one, less than one chunk), 143 nodes (a
ragged tail), every label width (3- and 5-bit fields across dwords, 8 bits on the hub graph),
17,424 nodes of 3-bit grid plans (hundreds of groups, many chunks), and 1, 5 and 77 chains (one
member; fewer than a thread's 4 x 4 block; a diagonal and an off-diagonal block, neither
full, at tile 64)."""
import numpy as np
import pytest

import census_ref
import overlap_ref
import pairdist_ref
import tally_ref
from cases import cases
from flipcomplexityempirical_amd import _lib, plancloud
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, grid_graph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8", "FLIPWALK_PWD_TILE",
            "FLIPWALK_PWD_CHUNK")

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


def graph_of(name):
    """(graph, seed plan, k, proposal mode, bounds, base) of a tests/cases.py case or of one of
    the two square grids test_gpu_overlap.py builds, built the same way."""
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
    return (ch.distance_matrix(), ch.distance_rowsums(), ch.nearest_plans())


def check_last(ch, a=None, b=None, X=None):
    """The last measurement against the reference on the plans ``X`` (default: what the handle
    holds now); returns (D, that measurement's histogram)."""
    X = ch.labels() if X is None else X
    a = np.arange(ch.n_chains) if a is None else a
    D, rs, near, h = pairdist_ref.measure(X, ch.dgraph.n, a, b)
    got_D, got_rs, got_near = read(ch)
    assert got_D.dtype == np.int32 and got_rs.dtype == np.int64 and got_near.dtype == np.int32
    assert got_D.shape == D.shape and np.array_equal(got_D, D)
    assert np.array_equal(got_rs, rs)
    assert np.array_equal(got_near, near)
    return D, h


def code(f, *a):
    with pytest.raises(_lib.FlipwalkError) as e:
        f(*a)
    return e.value.code


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_symmetric_matches_reference(gpu_lib, name, env, bits, n_chains, monkeypatch):
    ch = make(name, n_chains, env, monkeypatch)
    n, C = ch.dgraph.n, n_chains
    info = ch.pair_distance_info()
    assert (info["ma"], info["mb"], info["label_bits"], info["n_measured"]) == (0, 0, bits, 0)
    # 1. the seed plans: all equal
    ch.pair_distances()
    D, rs, near = read(ch)
    assert D.shape == (C, C) and not D.any() and not rs.any()
    want_near = [[0, 1 if i == 0 else 0] for i in range(C)] if C > 1 else [[-1, -1]]
    assert near.tolist() == want_near
    H = np.zeros(n + 1, np.uint64)
    H[0] = C * (C - 1) // 2
    assert np.array_equal(ch.pair_distance_hist(), H)
    info = ch.pair_distance_info()
    assert (info["ma"], info["mb"], info["symmetric"], info["n_measured"]) == (C, C, True, 1)
    # 2. 200 steps on
    ch.run(200)
    ch.pair_distances()
    D, h = check_last(ch)
    if C > 1:
        assert (D > 0).any()
    assert np.array_equal(D, D.T) and not np.diag(D).any()
    assert np.array_equal(ch.pair_distance_hist(), H + h)
    assert int(h.sum()) == C * (C - 1) // 2
    # the triangle inequality over all triples
    D64 = D.astype(np.int64)
    assert (D64[:, None, :] <= D64[:, :, None] + D64[None, :, :]).all()
    # 3. an independent route: the partner overlap of chain c with chain (c + s) % C
    for s in (1, 2, 5):
        ch.set_partners((np.arange(C) + s) % C)
        ch.overlap("partner")
        assert np.array_equal(ch.plan_distance(), D[np.arange(C), (np.arange(C) + s) % C])


def test_rectangular_and_transposed(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 77, {}, monkeypatch)
    n = ch.dgraph.n
    ch.run(200)
    a, b = np.arange(77), np.array([70, 41, 41, 9, 0])  # a duplicate, descending
    ch.pair_distances(a, b)
    D, h = check_last(ch, a, b)
    assert D.shape == (77, 5) and int(h.sum()) == 77 * 5
    assert np.array_equal(ch.pair_distance_hist(), h)
    info = ch.pair_distance_info()
    assert (info["ma"], info["mb"], info["symmetric"]) == (77, 5, False)
    j, d = plancloud.landmark_assign(D)
    assert np.array_equal(np.stack([d, j], axis=1), ch.nearest_plans())
    ch.pair_distances(b, a)
    Dt, ht = check_last(ch, b, a)
    assert np.array_equal(Dt, D.T)
    assert np.array_equal(ch.pair_distance_hist(), h + ht)
    # a list equal to all chains given as b is not the symmetric case: the diagonal counts
    ch.pair_distance_reset()
    ch.pair_distances(a, a)
    D2, h2 = check_last(ch, a, a)
    assert int(h2.sum()) == 77 * 77 and (ch.nearest_plans()[:, 0] == 0).all()


@pytest.mark.parametrize("name", ["grid11x13_k4", "grid40_k4"])
def test_forced_plans_give_the_default_plans_result(gpu_lib, name, monkeypatch):
    ch = make(name, 77, {}, monkeypatch)
    ch.run(200)
    ch.pair_distances()
    D, h = check_last(ch)
    want = read(ch)
    default = ch.pair_distance_info()
    assert default["tile"] == 64
    b = np.array([5, 76, 5, 33])
    ch.pair_distances(None, b)
    want_rect = read(ch)
    n_chunks = set()
    for tile in ("16", "32", None):
        for chunk in ("1", "2", "3", None):
            for key, val in (("FLIPWALK_PWD_TILE", tile), ("FLIPWALK_PWD_CHUNK", chunk)):
                if val is None:
                    monkeypatch.delenv(key, raising=False)
                else:
                    monkeypatch.setenv(key, val)
            ch.pair_distance_reset()
            ch.pair_distances()
            info = ch.pair_distance_info()
            assert info["tile"] == int(tile or 64)
            if chunk:
                assert info["chunk"] == int(chunk)
            elif tile is None:
                assert info["chunk"] == default["chunk"]
            n_chunks.add(-(-((ch.dgraph.n + 31) // 32) // info["chunk"]) % 2)
            for got, exp in zip(read(ch), want):
                assert np.array_equal(got, exp)
            assert np.array_equal(ch.pair_distance_hist(), h)
            ch.pair_distances(None, b)
            for got, exp in zip(read(ch), want_rect):
                assert np.array_equal(got, exp)
    assert n_chunks == {0, 1}  # walks that end in either staging buffer


def test_after_clone(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 77, {}, monkeypatch)
    ch.run(200)
    src = np.arange(77)
    src[7:] = src[7:] % 7  # chains 0..6 are the fixed points
    ch.clone(src)
    ch.pair_distances()
    D, _ = check_last(ch)
    assert not D[np.arange(77), src].any()
    cls, count = plancloud.distinct_plans(D)
    assert count == plancloud.distinct_plans(D[:7, :7])[1] <= 7
    assert count == len({row.tobytes() for row in ch.labels()})
    assert np.array_equal(cls[7:], cls[src[7:]])
    ch.run(50)
    ch.pair_distances()
    D, _ = check_last(ch)
    assert (D[np.arange(7, 77), src[7:]] > 0).any()


def test_stream_order(gpu_lib, monkeypatch):
    """run, measure, run with no wait between: the measurement sees the plans between the runs,
    which a second handle of the same seed run to that point holds."""
    ch = make("grid40_k4", 77, {}, monkeypatch)
    twin = make("grid40_k4", 77, {}, monkeypatch)
    ch.run_async(150)
    ch.pair_distances()
    ch.run_async(150)
    twin.run(150)
    between = twin.labels()
    D, _ = check_last(ch, X=between)
    assert (D > 0).any()
    assert not np.array_equal(ch.labels(), between)
    twin.run(150)
    assert np.array_equal(ch.labels(), twin.labels())  # the measurement moved nothing


def test_accumulation_reset_and_checkpoint(gpu_lib, monkeypatch, tmp_path):
    ch = make("grid11x13_k4", 9, {}, monkeypatch, seed=4)
    plain_keys = set(ch.checkpoint())
    assert "pair_distance_hist" not in plain_keys
    ch.run(100)
    never = make("grid11x13_k4", 9, {}, monkeypatch, seed=4)
    never.run(100)
    assert set(never.checkpoint()) == plain_keys  # a handle that never measured: today's keys
    ch.pair_distances()
    _, h1 = check_last(ch)
    ch.run(100)
    ch.pair_distances([8, 3, 1])
    _, h2 = check_last(ch, [8, 3, 1])
    assert np.array_equal(ch.pair_distance_hist(), h1 + h2)
    assert ch.pair_distance_info()["n_measured"] == 2
    assert set(ch.checkpoint()) == plain_keys | {"pair_distance_hist", "n_pair_distances"}
    path = str(tmp_path / "ck.npz")
    ch.save_checkpoint(path)
    resumed = Chains.from_checkpoint(ch.dgraph, path, ch.k)
    assert np.array_equal(resumed.pair_distance_hist(), h1 + h2)
    assert resumed.pair_distance_info()["n_measured"] == 2
    assert code(resumed.distance_matrix) == _lib.FW_ESTATE  # the matrix is not carried
    for c in (ch, resumed):
        c.run(50)
        c.pair_distances()
    assert np.array_equal(resumed.labels(), ch.labels())
    _, h3 = check_last(resumed)
    assert np.array_equal(resumed.pair_distance_hist(), h1 + h2 + h3)
    assert np.array_equal(ch.pair_distance_hist(), h1 + h2 + h3)
    assert resumed.pair_distance_info()["n_measured"] == ch.pair_distance_info()["n_measured"] == 3
    ch.reset_observables()  # leaves it alone
    assert np.array_equal(ch.pair_distance_hist(), h1 + h2 + h3)
    ch.pair_distance_reset()
    assert not ch.pair_distance_hist().any() and ch.pair_distance_info()["n_measured"] == 0
    assert plancloud.mean_pairwise(h3) == pytest.approx(
        ch.distance_matrix()[np.triu_indices(9, 1)].mean())


def test_refusals(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L = _lib.load()
    n = ch.dgraph.n
    for f in (ch.distance_matrix, ch.distance_rowsums, ch.nearest_plans):
        assert code(f) == _lib.FW_ESTATE
    assert not ch.pair_distance_hist().any()  # the histogram reads as zeros before any
    assert code(ch.pair_distances, [0, 5]) == _lib.FW_EINVAL
    assert code(ch.pair_distances, [-1]) == _lib.FW_EINVAL
    assert code(ch.pair_distances, [0, 1], [2, 7]) == _lib.FW_EINVAL
    assert code(ch.pair_distances, []) == _lib.FW_EINVAL
    with pytest.raises(ValueError):
        ch.pair_distances([0], [])
    ids = np.zeros(4, np.int32)
    assert L.fw_chains_pairdist_async(ch._h, None, 4, None, 0) == _lib.FW_EINVAL
    assert L.fw_chains_pairdist_async(ch._h, _lib.ptr(ids), 4, _lib.ptr(ids), 0) == _lib.FW_EINVAL
    big = np.zeros(16385, np.int32)  # 16385^2 > 2^28
    assert code(ch.pair_distances, big) == _lib.FW_EUNSUPPORTED
    assert code(ch.pair_distances, big, np.zeros(16384, np.int32)) == _lib.FW_EUNSUPPORTED
    assert ch.pair_distance_info()["n_measured"] == 0
    assert code(ch.distance_matrix) == _lib.FW_ESTATE  # a refused call measured nothing
    ch.pair_distances()
    for what, arr in ((_lib.PAIRDIST_MATRIX, np.zeros(25, np.int32)),
                      (_lib.PAIRDIST_ROWSUM, np.zeros(5, np.int64)),
                      (_lib.PAIRDIST_NEAREST, np.zeros(10, np.int32)),
                      (_lib.PAIRDIST_HIST, np.zeros(n + 1, np.uint64))):
        assert L.fw_chains_read_pairdist(ch._h, what, _lib.ptr(arr), arr.nbytes - 1) == _lib.FW_EINVAL
        assert L.fw_chains_read_pairdist(ch._h, what, _lib.ptr(arr), arr.nbytes) == _lib.FW_OK
        rc = L.fw_chains_write_pairdist(ch._h, what, _lib.ptr(arr), arr.nbytes)
        assert rc == (_lib.FW_OK if what == _lib.PAIRDIST_HIST else _lib.FW_EINVAL)
    buf = np.zeros(n + 1, np.uint64)
    assert L.fw_chains_read_pairdist(ch._h, 4, _lib.ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_write_pairdist(ch._h, _lib.PAIRDIST_HIST, _lib.ptr(buf), buf.nbytes - 1) == \
        _lib.FW_EINVAL


def test_coexists_with_tally_overlap_and_census(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 77, {}, monkeypatch)
    n, k = ch.dgraph.n, ch.k
    cols = np.random.default_rng(3).integers(0, 1000, (2, n))
    ch.set_columns(cols)
    ch.set_reference()
    ch.enable_census()
    ch.run(200)
    ch.tally()
    ch.overlap()
    ch.census()
    ch.pair_distances()
    ch.tally()
    ch.overlap()
    ch.census()
    X = ch.labels()
    check_last(ch)
    assert np.array_equal(ch.tallies(), tally_ref.sums(X, cols, k))
    O, dist = overlap_ref.overlap(ch.reference(), X, k)
    assert np.array_equal(ch.overlap_matrix(), O) and np.array_equal(ch.plan_distance(), dist)
    assert np.array_equal(ch.distance_hist(), 2 * overlap_ref.dist_hist(dist, n))
    want = census_ref.census(ch.graph, X, k)
    assert np.array_equal(ch.node_occupancy(), 2 * want["occ"])
    assert np.array_equal(ch.edge_cut_counts(), 2 * want["ecut"])
    assert np.array_equal(ch.boundary_counts(), 2 * want["bnd"])
    assert ch.tally_info()["n_tallied"] == 2 and ch.census_info()["n_measured"] == 2
    check_last(ch)  # and the other steps left the matrix alone


def test_run_sampled_pairs(gpu_lib, monkeypatch):
    """One symmetric measurement per sample; the histogram is the sum over the samples,
    recomputed from a second handle stepped identically."""
    ch = make("grid16x24_k8", 5, {}, monkeypatch)
    twin = make("grid16x24_k8", 5, {}, monkeypatch)
    for c in (ch, twin):
        c.enable_series(8)
    ch.run_sampled(60, 4, pairs=True)
    H = np.zeros(ch.dgraph.n + 1, np.uint64)
    for _ in range(4):
        twin.run_sampled(60, 1)
        H += pairdist_ref.measure(twin.labels(), ch.dgraph.n, np.arange(5))[3]
    assert np.array_equal(ch.labels(), twin.labels())
    assert np.array_equal(ch.pair_distance_hist(), H) and int(H.sum()) == 4 * 10
    assert ch.pair_distance_info()["n_measured"] == 4
    check_last(ch)
    # a member list instead of all chains
    ch.run_sampled(60, 1, pairs=[4, 0, 2])
    check_last(ch, [4, 0, 2])
    assert ch.pair_distance_info()["n_measured"] == 5
    # off by default
    ch.run_sampled(60, 1)
    assert ch.pair_distance_info()["n_measured"] == 5
