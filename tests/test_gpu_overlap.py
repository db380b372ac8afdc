"""Plan overlap and Hamming distance on the GPU (fw_chains_set_reference / fw_chains_set_partners
/ fw_chains_overlap_async) against the numpy restatement in overlap_ref.py.  Every comparison
is exact (``np.array_equal``) and is made against ``reference()`` and ``labels()`` read at the
same point.  The shapes are test_gpu_tally.py's WIDTH_CASES: the smallest that reach every
label width, a group set under one 64-lane step, a ragged tail and a partly filled workgroup."""
import numpy as np
import pytest

import overlap_ref
from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, grid_graph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
ENV_KEYS = ("FLIPWALK_NO_GRID16", "FLIPWALK_CSR_LB", "FLIPWALK_BIG_K8", "FLIPWALK_OVL_NW")

# (case, environment, label bits expected, chains): test_gpu_tally.py's WIDTH_CASES
WIDTH_CASES = [
    ("grid7x9_k3_cut", {}, 2, 5),          # 63 nodes: two groups, under one 64-lane step
    ("grid11x13_k4", {}, 2, 77),           # 143 nodes: a ragged tail; chains fill no workgroup
    ("grid40x3_k2_cut", {}, 4, 1),         # 4-bit, one chain
    ("grid40_k4", {}, 2, 77),              # 1,600 nodes
    ("grid40_k4", {"FLIPWALK_NO_GRID16": "1", "FLIPWALK_CSR_LB": "3"}, 3, 5),
    ("grid16x24_k8", {}, 4, 5),
    ("delaunay3k_k31", {"FLIPWALK_CSR_LB": "5"}, 5, 5),   # 961 bins, fields across dwords
    ("delaunay3k_k18", {"FLIPWALK_CSR_LB": "8"}, 8, 77),
    ("hub_k3", {}, 8, 5),
    ("big132_k8", {"FLIPWALK_BIG_K8": "1"}, 3, 5),  # 17,424 nodes, 3-bit grid-kernel plans
]
IDS = [f"{c[0]}-lb{c[2]}-c{c[3]}" for c in WIDTH_CASES]


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


def check_last(ch, ref=None, groups=None, n_groups=1):
    """The last measurement against the reference on what the handle holds now; returns
    (O, dist, that measurement's histogram).  ``ref``: the plans compared with (default: the
    stored reference)."""
    ref = ch.reference() if ref is None else ref
    O, dist = overlap_ref.overlap(ref, ch.labels(), ch.k)
    got_O, got_d = ch.overlap_matrix(), ch.plan_distance()
    assert got_O.dtype == np.int64 and got_d.dtype == np.int32
    assert np.array_equal(got_O, O)
    assert np.array_equal(got_d, dist)
    return O, dist, overlap_ref.dist_hist(dist, ch.dgraph.n, groups, n_groups)


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_overlap_matches_reference(gpu_lib, name, env, bits, n_chains, monkeypatch):
    ch = make(name, n_chains, env, monkeypatch)
    n, k = ch.dgraph.n, ch.k
    seed_plan = np.asarray(graph_of(name)[1], np.int16)
    assert ch.overlap_info() == {"reference": "none", "label_bits": bits, "n_groups": 1,
                                 "partners": False, "n_measured": 0}
    # 1. a snapshot of the seed plans, compared with themselves
    ch.set_reference()
    ch.overlap()
    info = ch.overlap_info()
    assert (info["reference"], info["label_bits"], info["n_measured"]) == ("per_chain", bits, 1)
    assert not ch.plan_distance().any()
    sizes = np.bincount(seed_plan, minlength=k)
    assert np.array_equal(ch.overlap_matrix(), np.tile(np.diag(sizes), (n_chains, 1, 1)))
    # 2. 200 steps on
    ch.run(200)
    ch.overlap()
    assert np.array_equal(ch.reference(), np.tile(seed_plan, (n_chains, 1)))
    O, dist, h = check_last(ch)
    assert (dist > 0).any()
    H = overlap_ref.dist_hist(np.zeros(n_chains), n) + h
    assert np.array_equal(ch.distance_hist(), H)
    assert ch.overlap_info()["n_measured"] == 2
    # 4. the invariants
    ch.set_geometry()
    ch.geometry()
    assert np.array_equal(O.sum(axis=2), np.tile(sizes, (n_chains, 1)))
    assert np.array_equal(ch.overlap_matrix().sum(axis=1), ch.district_geometry()[..., 0])
    assert (ch.overlap_matrix().sum(axis=(1, 2)) == n).all()
    assert np.array_equal(ch.plan_distance(), n - np.trace(ch.overlap_matrix(), axis1=1, axis2=2))
    # 3. independent uniform labels per node: many pairs in every 32-node group
    rng = np.random.default_rng(1000 * bits + n_chains)
    for shape, kind in (((n,), "shared"), ((n_chains, n), "per_chain")):
        ref = rng.integers(0, k, shape).astype(np.int16)
        ch.set_reference(ref)
        info = ch.overlap_info()
        assert (info["reference"], info["n_measured"]) == (kind, 0)
        assert not ch.distance_hist().any()
        ch.overlap()
        assert np.array_equal(ch.reference(), ref)
        O, dist, h = check_last(ch, ref)
        assert np.array_equal(ch.distance_hist(), h)
        rows = np.broadcast_to(ref, (n_chains, n))
        assert np.array_equal(O.sum(axis=2), np.stack([np.bincount(r, minlength=k) for r in rows]))


TALLY_CASES = [c for c in WIDTH_CASES if c[0] in ("grid11x13_k4", "grid16x24_k8", "hub_k3") or
               (c[0] == "grid40_k4" and c[2] == 3)]


@pytest.mark.parametrize("name,env,bits,n_chains", TALLY_CASES,
                         ids=[f"{c[0]}-lb{c[2]}" for c in TALLY_CASES])
def test_shared_reference_equals_an_indicator_tally(gpu_lib, name, env, bits, n_chains,
                                                    monkeypatch):
    """An independent route to the same table: with the k columns the indicators of the
    reference's districts, tallies()[c, d, e] counts the nodes the reference labels d and chain
    c labels e."""
    ch = make(name, n_chains, env, monkeypatch)
    assert ch.k <= 8 and sorted(c[2] for c in TALLY_CASES) == [2, 3, 4, 8]
    ref = np.random.default_rng(bits).integers(0, ch.k, ch.dgraph.n).astype(np.int16)
    ch.set_columns(np.stack([(ref == d) for d in range(ch.k)]).astype(np.int64))
    ch.set_reference(ref)
    ch.run(200)
    ch.tally()
    ch.overlap()
    assert ch.overlap_info()["label_bits"] == bits
    assert np.array_equal(ch.overlap_matrix(), ch.tallies())
    assert ch.plan_distance().all()  # a random labelling is far from every plan


def test_partner_mode(gpu_lib, monkeypatch):
    """77 chains (five workgroups of 16 waves): partners cross workgroups."""
    ch = make("grid11x13_k4", 77, {}, monkeypatch)
    C, n = 77, ch.dgraph.n
    ch.run(200)
    lab = ch.labels()
    H = 0
    perm = np.random.default_rng(5).permutation(C)
    for partner, want in ((None, (np.arange(C) + 1) % C), (perm, perm),
                          (np.arange(C), np.arange(C))):
        ch.set_partners(partner)
        assert np.array_equal(ch.partners, want)
        ch.overlap("partner")
        O, dist, h = check_last(ch, lab[want])
        H = H + h
        assert dist.any() == (not np.array_equal(want, np.arange(C)))
    assert np.array_equal(ch.distance_hist(), H)  # set_partners leaves the histogram alone
    info = ch.overlap_info()
    assert (info["reference"], info["partners"], info["n_measured"]) == ("none", True, 3)
    # partner[c] = c: distance 0 (the permutation's fixed points are there as well)
    assert int(ch.distance_hist()[0, 0]) == C + int((perm == np.arange(C)).sum())
    one = make("grid11x13_k4", 1, {}, monkeypatch)
    with pytest.raises(ValueError):
        one.set_partners()


def test_snapshot_is_taken_in_stream_order(gpu_lib, monkeypatch):
    """run_async(100), set_reference(), run_async(100), overlap() with no sync in between: the
    reference is the plans after 100 steps, the current plans those after 200."""
    a = make("grid40_k4", 77, {}, monkeypatch)
    b = make("grid40_k4", 77, {}, monkeypatch)
    a.run_async(100)
    a.set_reference()
    a.run_async(100)
    a.overlap()
    b.run(100)
    at100 = b.labels()
    b.run(100)
    at200 = b.labels()
    O, dist = overlap_ref.overlap(at100, at200, a.k)
    assert np.array_equal(a.overlap_matrix(), O) and np.array_equal(a.plan_distance(), dist)
    assert np.array_equal(a.reference(), at100) and np.array_equal(a.labels(), at200)
    assert dist.any() and not np.array_equal(at100, np.tile(graph_of("grid40_k4")[1], (77, 1)))


def test_histogram_by_rung(gpu_lib, monkeypatch):
    """8 rungs x 4 sets, run_tempered(20, 6, overlap=True): a plan's distance is binned under
    the rung it has just run on; the reference replays the rounds synchronously and reads
    labels() and rungs() before each exchange."""
    a, b = (make("grid12_k4_pairs", 32, {}, monkeypatch, seed=9) for _ in range(2))
    for ch in (a, b):
        ch.set_ladder(np.geomspace(0.7, 1.4, 8))
    n = a.dgraph.n
    a.set_reference()
    seed_plan = a.reference()
    assert a.overlap_info()["n_groups"] == 8
    a.run_tempered(20, 6, overlap=True)
    H, moved = 0, False
    for i in range(6):
        b.run(20)
        rungs = b.rungs()
        moved = moved or not np.array_equal(rungs, np.arange(32) % 8)
        O, dist = overlap_ref.overlap(seed_plan, b.labels(), b.k)
        H = H + overlap_ref.dist_hist(dist, n, rungs, 8)
        b.exchange(i)
        b.sync()
    assert moved and dist.any()
    got = a.distance_hist()
    assert got.shape == (8, n + 1) and np.array_equal(got, H)
    assert (got.sum(axis=1) == 6 * 4).all()  # rounds x sets on every rung
    assert np.array_equal(a.overlap_matrix(), O) and np.array_equal(a.plan_distance(), dist)
    assert a.overlap_info()["n_measured"] == 6
    # set_ladder afterwards re-sizes the histogram and zeroes it
    a.set_ladder(np.geomspace(0.7, 1.4, 4))
    assert a.distance_hist().shape == (4, n + 1) and not a.distance_hist().any()
    a.overlap()
    _, _, h = check_last(a, groups=a.rungs(), n_groups=4)
    assert np.array_equal(a.distance_hist(), h)


@pytest.mark.parametrize("nw", ["1", "3"])
def test_forced_waves_per_workgroup(gpu_lib, nw, monkeypatch):
    """FLIPWALK_OVL_NW = 1, and 3: 77 chains leave the last workgroup partly filled."""
    ch = make("grid11x13_k4", 77, {"FLIPWALK_OVL_NW": nw}, monkeypatch)
    ch.run(200)
    ref = np.random.default_rng(int(nw)).integers(0, ch.k, (77, ch.dgraph.n)).astype(np.int16)
    ch.set_reference(ref)
    ch.overlap()
    check_last(ch, ref)
    ch.set_partners()
    ch.overlap("partner")
    check_last(ch, ch.labels()[ch.partners])


def test_refusals_and_resets(gpu_lib, monkeypatch):
    ch = make("grid11x13_k4", 5, {}, monkeypatch)
    L = _lib.load()
    n, k, C = ch.dgraph.n, ch.k, 5

    def code(f, *a):
        with pytest.raises(_lib.FlipwalkError) as e:
            f(*a)
        return e.value.code

    O = np.zeros((C, k, k), np.int64)
    # before a reference and before partners
    assert code(ch.overlap) == _lib.FW_ESTATE
    assert code(ch.overlap, "partner") == _lib.FW_ESTATE
    assert L.fw_chains_overlap_async(ch._h, 2) == _lib.FW_EINVAL
    assert L.fw_chains_read_overlap(ch._h, _lib.OVERLAP_MATRIX, _lib.ptr(O), O.nbytes) == \
        _lib.FW_ESTATE
    # labels and partners out of range: refused on the host, nothing is set
    for bad in (k, -1):
        lab = np.zeros(n, np.int16)
        lab[n // 2] = bad
        assert L.fw_chains_set_reference(ch._h, _lib.ptr(lab), 0) == _lib.FW_EINVAL
        labs = np.zeros((C, n), np.int16)
        labs[C - 1, n - 1] = bad
        assert L.fw_chains_set_reference(ch._h, _lib.ptr(labs), 1) == _lib.FW_EINVAL
        with pytest.raises(ValueError):
            ch.set_reference(lab)
    for bad in (C, -1):
        p = np.arange(C, dtype=np.int32)
        p[2] = bad
        assert L.fw_chains_set_partners(ch._h, _lib.ptr(p)) == _lib.FW_EINVAL
        with pytest.raises(ValueError):
            ch.set_partners(p)
    assert ch.overlap_info()["reference"] == "none" and not ch.overlap_info()["partners"]
    assert code(ch.overlap) == _lib.FW_ESTATE
    # a reference, nothing measured yet
    ch.set_reference()
    assert code(ch.overlap_matrix) == _lib.FW_ESTATE
    assert code(ch.plan_distance) == _lib.FW_ESTATE
    assert not ch.distance_hist().any()
    assert code(ch.overlap, "partner") == _lib.FW_ESTATE  # a reference is no partner array
    ch.run(200)
    ch.overlap()
    _, _, h = check_last(ch)
    # short buffers, unknown kinds, the kinds that cannot be written
    hist = ch.distance_hist()
    dist = np.zeros(C, np.int32)
    refb = np.zeros((C, n), np.int16)
    for what, buf in ((_lib.OVERLAP_MATRIX, O), (_lib.OVERLAP_DIST, dist),
                      (_lib.OVERLAP_HIST, hist), (_lib.OVERLAP_REF, refb)):
        assert L.fw_chains_read_overlap(ch._h, what, _lib.ptr(buf), buf.nbytes - 1) == \
            _lib.FW_EINVAL
        assert L.fw_chains_read_overlap(ch._h, what, _lib.ptr(buf), buf.nbytes) == _lib.FW_OK
    assert L.fw_chains_read_overlap(ch._h, 7, _lib.ptr(O), O.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_write_overlap(ch._h, _lib.OVERLAP_HIST, _lib.ptr(hist),
                                     hist.nbytes - 1) == _lib.FW_EINVAL
    assert L.fw_chains_write_overlap(ch._h, _lib.OVERLAP_MATRIX, _lib.ptr(O), O.nbytes) == \
        _lib.FW_EINVAL
    # reset_observables leaves the overlap alone; overlap_reset zeroes histogram and count
    ch.reset_observables()
    assert np.array_equal(ch.distance_hist(), h) and ch.overlap_info()["n_measured"] == 1
    check_last(ch)
    ch.overlap_reset()
    assert not ch.distance_hist().any() and ch.overlap_info()["n_measured"] == 0
    ch.overlap()
    assert np.array_equal(ch.distance_hist(), h) and ch.overlap_info()["n_measured"] == 1
    # what MATRIX holds is recorded per kind: new partners invalidate a partner measurement,
    # not one against the reference; a new reference invalidates either
    ch.set_partners()
    check_last(ch)
    ch.overlap("partner")
    check_last(ch, ch.labels()[ch.partners])
    ch.set_partners(np.arange(C))
    assert code(ch.overlap_matrix) == _lib.FW_ESTATE
    ch.overlap("partner")
    assert not ch.plan_distance().any()
    ch.set_reference()
    assert code(ch.plan_distance) == _lib.FW_ESTATE
    assert ch.overlap_info()["n_measured"] == 0 and not ch.distance_hist().any()


def test_checkpoint_carries_the_overlap(gpu_lib, monkeypatch, tmp_path):
    whole = make("grid11x13_k4", 9, {}, monkeypatch, seed=4)
    whole.run(100)
    whole.set_reference()
    whole.set_partners(np.random.default_rng(2).permutation(9))
    for _ in range(2):
        whole.run(100)
        whole.overlap()
    whole.overlap("partner")
    path = str(tmp_path / "ck.npz")
    whole.save_checkpoint(path)
    resumed = Chains.from_checkpoint(whole.dgraph, path, whole.k)
    assert np.array_equal(resumed.reference(), whole.reference())
    assert np.array_equal(resumed.partners, whole.partners)
    assert np.array_equal(resumed.distance_hist(), whole.distance_hist())
    assert whole.distance_hist().sum() == 27
    assert resumed.overlap_info() == whole.overlap_info()
    assert resumed.overlap_info()["n_measured"] == 3
    for ch in (whole, resumed):
        ch.run(100)
        ch.overlap()
    assert np.array_equal(resumed.overlap_matrix(), whole.overlap_matrix())
    assert np.array_equal(resumed.plan_distance(), whole.plan_distance())
    check_last(resumed)
    for ch in (whole, resumed):
        ch.overlap("partner")
    assert np.array_equal(resumed.overlap_matrix(), whole.overlap_matrix())
    assert np.array_equal(resumed.distance_hist(), whole.distance_hist())
    assert resumed.overlap_info()["n_measured"] == whole.overlap_info()["n_measured"] == 5
    # a histogram of another shape is refused
    ck = whole.checkpoint()
    ck["distance_hist"] = np.zeros((2, whole.dgraph.n + 1), np.uint64)
    with pytest.raises(ValueError):
        resumed.restore(ck)


def test_overlap_shares_a_handle_with_tally_and_geometry(gpu_lib, monkeypatch):
    """run_sampled(tally=True, geometry=True, overlap=True) ends with the plans, stats, series,
    tallies and geometry of the same run without the overlap."""
    both = make("grid11x13_k4", 77, {}, monkeypatch)
    plain = make("grid11x13_k4", 77, {}, monkeypatch)
    cols = np.random.default_rng(1).integers(0, 100, (3, both.dgraph.n))
    for ch in (both, plain):
        ch.set_columns(cols)
        ch.set_geometry()
        ch.enable_series(8)
    both.set_reference()
    both.set_partners()
    both.run_sampled(60, 4, tally=True, geometry=True, overlap=True)
    both.overlap("partner")
    plain.run_sampled(60, 4, tally=True, geometry=True)
    assert both.overlap_info()["n_measured"] == 5
    assert both.tally_info()["n_tallied"] == both.geometry_info()["n_measured"] == 4
    assert int(both.distance_hist().sum()) == 5 * 77
    assert np.array_equal(both.labels(), plain.labels())
    assert both.stats().tobytes() == plain.stats().tobytes()
    assert np.array_equal(both.series("cut"), plain.series("cut"))
    assert np.array_equal(both.tallies(), plain.tallies())
    assert np.array_equal(both.district_geometry(), plain.district_geometry())
    assert np.array_equal(both.geometry_hist(), plain.geometry_hist())
    check_last(both, both.labels()[both.partners])
