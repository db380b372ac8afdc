"""Resampling plans across chains on the GPU (fw_chains_clone_async / fw_chains_resample_async)
against the integer restatement in resample_ref.py and against the host route {read, numpy
gather, fw_chains_write} on a second handle of the same seed.  Every comparison is exact
(``np.array_equal``): labels, every stats field (the bytes of sum_invb included), populations and
both histograms.  The shapes are test_gpu_tally.py's WIDTH_CASES (all five label widths, 63
nodes, ragged tails, 1 / 5 / 77 chains, both kernels), plus 2,500 chains where the map kernel's
1,024-chain tiles must carry their sums."""
import numpy as np
import pytest

import overlap_ref
import resample_ref
from cases import cases
from flipcomplexityempirical_amd import _lib, population
from flipcomplexityempirical_amd._lib import ptr
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph, population_bounds
from flipcomplexityempirical_amd.graph import block_seed, boundary_flags, grid_graph

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
SEED = 77


def graph_of(name):
    """(graph, seed plan, k, proposal mode, bounds, base), as test_gpu_overlap.py builds them."""
    if name in ("grid40_k4", "big132_k8"):
        side, blocks, k = (40, (2, 2), 4) if name == "grid40_k4" else (132, (2, 4), 8)
        g = grid_graph(side, side)
        return g, block_seed(side, side, *blocks), k, 1, population_bounds(g.total_pop, k, 0.05), 0.5
    c = CASES[name]
    return c.graph, c.init, c.k, c.mode, c.bounds, c.base


def make(name, n_chains, env=None, monkeypatch=None, seed=SEED, init=None, **kw):
    if monkeypatch is not None:
        for key in ENV_KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in (env or {}).items():
            monkeypatch.setenv(key, val)
    g, init0, k, mode, bounds, base = graph_of(name)
    kw.setdefault("base", base)
    return Chains(DeviceGraph(g), n_chains, k, init0 if init is None else init, proposal=mode,
                  pop_bounds=bounds, seed=seed, **kw)


def state(ch):
    return {"labels": ch.labels(), "stats": ch.stats(), "pops": ch.pops(),
            "hist_cut": ch.hist_cut(), "hist_b": ch.hist_b()}


def assert_same(a, b):
    """Two handles' states, exactly: every stats field by its bytes."""
    sa, sb = state(a), state(b)
    for key in ("labels", "pops", "hist_cut", "hist_b"):
        assert np.array_equal(sa[key], sb[key]), key
    for f in sa["stats"].dtype.names:
        x, y = np.ascontiguousarray(sa["stats"][f]), np.ascontiguousarray(sb["stats"][f])
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f
    return sa


def write(ch, what, a):
    a = np.ascontiguousarray(a)
    _lib.check(_lib.load().fw_chains_write(ch._h, what, ptr(a), a.nbytes))


def host_route(ch, src):
    """The route the clone replaces: read, gather on the host, write back."""
    waits = ch.waits() if ch.waits_on else None
    lab, st, _, w, _ = resample_ref.gather(src, ch.labels(), ch.stats(), waits=waits)
    write(ch, _lib.READ_LABELS, lab)
    write(ch, _lib.READ_STATS, st)
    if w is not None:
        write(ch, _lib.READ_WAITS, w)


def clone_map(C, rng):
    """Fixed points, several clones of one source, destinations in every workgroup of the
    gather (4 chains each): about C / 8 sources, 60% of the other chains replaced."""
    src = np.arange(C, dtype=np.int32)
    if C < 2:
        return src
    sources = np.sort(rng.choice(C, max(1, C // 8), replace=False))
    others = np.setdiff1d(np.arange(C), sources)
    take = others[rng.random(len(others)) < 0.6]
    if len(take) < 2:
        take = others[:2]
    src[take] = rng.choice(sources, len(take))
    src[take[:2]] = sources[0]  # one source cloned at least twice
    return src


def check_gathered(ch, before, src):
    """The handle holds the gather of ``before`` (a state() taken just before) by src."""
    lab, st, pops, _, _ = resample_ref.gather(src, before["labels"], before["stats"], before["pops"])
    assert np.array_equal(ch.labels(), lab)
    assert np.array_equal(ch.pops(), pops)
    got = ch.stats()
    for f in got.dtype.names:
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8),
                              np.ascontiguousarray(st[f]).view(np.uint8)), f


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_clone_equals_the_host_route_after_a_run(gpu_lib, name, env, bits, n_chains, monkeypatch):
    a, b = (make(name, n_chains, env, monkeypatch) for _ in range(2))
    assert a.overlap_info()["label_bits"] == bits
    assert np.array_equal(a.families(), np.arange(n_chains))
    src = clone_map(n_chains, np.random.default_rng(n_chains + bits))
    for ch in (a, b):
        ch.run(200)
    before = state(a)
    a.clone(src)
    check_gathered(a, before, src)
    assert np.array_equal(a.last_sources(), src) and np.array_equal(a.families(), src)
    info = a.resample_info()
    assert (info["clones"], info["n_resampled"], info["round"]) == (int((src != np.arange(n_chains)).sum()), 0, -1)
    host_route(b, src)
    assert_same(a, b)
    for ch in (a, b):
        ch.run(200)
    after = assert_same(a, b)
    if n_chains > 1:  # clones diverge at once: own chain id, own attempt counter
        i = int(np.flatnonzero(src != np.arange(n_chains))[0])
        assert not np.array_equal(after["labels"][i], after["labels"][src[i]])
    # a second clone: families compose
    src2 = clone_map(n_chains, np.random.default_rng(1 + n_chains))
    a.clone(src2)
    assert np.array_equal(a.families(), src[src2])


@pytest.mark.parametrize("name,n_chains", [("grid11x13_k4", 77), ("grid16x24_k8", 5), ("hub_k3", 5)])
def test_clone_before_the_first_run(gpu_lib, name, n_chains, monkeypatch):
    """Equals a handle created with the per-chain initial plans init[src[i]]; every chain yields
    its new initial plan once."""
    helper = make(name, n_chains, {}, monkeypatch, seed=5)
    helper.run(200)
    init = helper.labels()
    src = clone_map(n_chains, np.random.default_rng(3))
    a = make(name, n_chains, init=init)
    b = make(name, n_chains, init=init[src])
    a.clone(src)
    assert np.array_equal(a.labels(), init[src])
    for ch in (a, b):
        ch.run(200)
    st = assert_same(a, b)
    assert (st["stats"]["yields"] == 201).all()


RESAMPLE_BASES = {+1: 1.3, -1: 1 / 1.5}


def resample_and_check(a, b0, b1, round, n_resampled=1, families=None, clones0=0):
    """a.resample against resample_ref on the stats read just before; returns the reference."""
    C = a.n_chains
    before = state(a)
    q, sign = population.weight_table(b0, b1, a.dgraph.n_edges)
    ref = resample_ref.resample_map(before["stats"]["cut"], q, sign,
                                    resample_ref.draw_u(a.seed, round, a.chain_id0))
    a.resample(b0, b1, round=round)
    assert np.array_equal(a.last_weights(), ref["W"])
    assert np.array_equal(a.last_sources(), ref["src"])
    info = a.resample_info()
    want = {"n_resampled": n_resampled, "round": round, "T": ref["T"], "S2": ref["S2"],
            "cref": ref["cref"], "survivors": ref["survivors"],
            "max_offspring": ref["max_offspring"], "clones": clones0 + C - ref["survivors"]}
    assert info == want
    fam = np.arange(C) if families is None else families
    assert np.array_equal(a.families(), fam[ref["src"]])
    check_gathered(a, before, ref["src"])
    return ref


@pytest.mark.parametrize("name,env,bits,n_chains", WIDTH_CASES, ids=IDS)
def test_resample_equals_the_reference_and_the_host_route(gpu_lib, name, env, bits, n_chains,
                                                          monkeypatch):
    a, b = (make(name, n_chains, env, monkeypatch) for _ in range(2))
    base = graph_of(name)[5]
    for ch in (a, b):
        ch.run(200)
    ref = resample_and_check(a, base, base * RESAMPLE_BASES[+1], round=3)
    assert a.resample_round == 4
    host_route(b, ref["src"])
    for ch in (a, b):
        ch.run(200)
    assert_same(a, b)


@pytest.mark.parametrize("n_chains", [77, 2500])
@pytest.mark.parametrize("b0,b1", [(1.0, RESAMPLE_BASES[-1]), (1.0, 50.0), (50.0, 1.0)],
                         ids=["down", "steep-up", "steep-down"])
def test_resample_signs_rounds_and_steep_tables(gpu_lib, n_chains, b0, b1, monkeypatch):
    """Both signs; a table that zeroes most weights; two rounds draw different u; the same round
    on a same-seed handle gives the same map; 2,500 chains span three tiles of the scans."""
    a, b, c = (make("grid40_k4", n_chains, {}, monkeypatch) for _ in range(3))
    for ch in (a, b, c):
        ch.run(200)
    ra = resample_and_check(a, b0, b1, round=0)
    rb = resample_and_check(b, b0, b1, round=1)
    c.resample(b0, b1, round=0)
    assert np.array_equal(c.last_sources(), ra["src"])
    assert resample_ref.draw_u(SEED, 0, 0) != resample_ref.draw_u(SEED, 1, 0)
    assert np.array_equal(ra["W"], rb["W"])  # the same population: only the offset differs
    assert ra["survivors"] < n_chains
    if max(b0, b1) == 50.0:
        assert (ra["W"] == 0).sum() > n_chains // 2 and ra["max_offspring"] > 1
    # a second resample on the resampled population: the counters and the families go on
    a.run(50)
    resample_and_check(a, b1, b0, round=1, n_resampled=2, families=ra["src"],
                       clones0=n_chains - ra["survivors"])


def test_boundary_accept_counts_follow_the_plans(gpu_lib, monkeypatch):
    g = graph_of("grid12_k4_cut")[0]
    flags = boundary_flags(g)
    a, b = (make("grid12_k4_cut", 77, {}, monkeypatch) for _ in range(2))
    src = clone_map(77, np.random.default_rng(8))
    for ch in (a, b):
        ch.set_accept("boundary", flags)
        ch.run(200)
    a.clone(src)
    host_route(b, src)  # the labels write recounts the flagged nodes from the plans
    for ch in (a, b):
        ch.run(300)
    st = assert_same(a, b)
    assert st["stats"]["accepts"].sum() > 0


def test_sampled_wait_draw_follows_the_plan(gpu_lib, monkeypatch):
    a, b = (make("grid12_k4_pairs", 77, {}, monkeypatch) for _ in range(2))
    src = clone_map(77, np.random.default_rng(9))
    for ch in (a, b):
        ch.enable_sampled_waits()
        ch.run(200)
    w = a.waits()
    a.clone(src)
    got = a.waits()
    assert np.array_equal(got[:, 1], w[src, 1]) and np.array_equal(got[:, 0], w[:, 0])
    assert not np.array_equal(w[src, 1], w[:, 1])
    host_route(b, src)
    for ch in (a, b):
        ch.run(200)
    assert_same(a, b)
    assert np.array_equal(a.waits(), b.waits())


def test_measurements_after_a_clone_see_the_new_plans(gpu_lib, monkeypatch):
    a = make("grid11x13_k4", 77, {}, monkeypatch)
    C, n, k = 77, a.dgraph.n, a.k
    cols = np.random.default_rng(4).integers(0, 50, (2, n)).astype(np.int64)
    a.set_columns(cols)
    a.set_geometry()
    a.enable_series(4)
    a.run(200)
    a.set_reference()  # a snapshot before the clone
    ref0, cut0 = a.reference(), a.stats()["cut"]
    src = clone_map(C, np.random.default_rng(10))
    a.clone(src)
    a.tally()
    a.geometry()
    a.overlap()
    a.record()
    lab = a.labels()
    assert np.array_equal(lab, ref0[src])
    assert np.array_equal(a.reference(), ref0)  # the reference stays with the chain
    T = np.stack([[np.bincount(l, weights=c, minlength=k) for c in cols] for l in lab]).astype(np.int64)
    assert np.array_equal(a.tallies(), T)
    assert np.array_equal(a.district_geometry()[..., 0],
                          np.stack([np.bincount(l, minlength=k) for l in lab]))
    O, dist = overlap_ref.overlap(ref0, lab, k)
    assert np.array_equal(a.overlap_matrix(), O) and np.array_equal(a.plan_distance(), dist)
    assert dist[src != np.arange(C)].any() and not dist[src == np.arange(C)].any()
    assert np.array_equal(a.series("cut")[0], cut0[src])


def test_refusals(gpu_lib, monkeypatch):
    L = _lib.load()
    a = make("grid11x13_k4", 5, {}, monkeypatch)
    E = a.dgraph.n_edges

    def code(fn, *args):
        with pytest.raises(_lib.FlipwalkError) as e:
            fn(*args)
        return e.value.code

    with pytest.raises(_lib.FlipwalkError):  # nothing cloned yet
        a.last_sources()
    with pytest.raises(_lib.FlipwalkError):
        a.last_weights()
    assert code(a.clone, [0, 1, 5, 3, 4]) == _lib.FW_EINVAL      # out of range
    assert code(a.clone, [0, -1, 2, 3, 4]) == _lib.FW_EINVAL
    assert code(a.clone, [1, 2, 2, 3, 4]) == _lib.FW_EINVAL      # 1 is not a fixed point
    with pytest.raises(ValueError):
        a.clone([0, 1, 2])
    q, sign = population.weight_table(1.0, 1.5, E)
    bad0, rising = q.copy(), q.copy()
    bad0[0] -= 1
    rising[5] = rising[4] + 1
    for table, s, rnd in ((bad0, 1, 0), (rising, 1, 0), (q, 0, 0), (q, 2, 0), (q, 1, -1),
                          (q, 1, 1 << 32)):
        assert L.fw_chains_resample_async(a._h, ptr(table), s, rnd) == _lib.FW_EINVAL
    assert L.fw_chains_resample_async(a._h, None, 1, 0) == _lib.FW_EINVAL
    assert a.resample_info()["n_resampled"] == 0 and np.array_equal(a.families(), np.arange(5))
    buf = np.zeros(5, np.int32)
    assert L.fw_chains_read_resample(a._h, 7, ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_read_resample(a._h, _lib.RESAMPLE_FAMILY, ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
    assert L.fw_chains_write_resample(a._h, _lib.RESAMPLE_SRC, ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_write_resample(a._h, _lib.RESAMPLE_FAMILY, ptr(buf), buf.nbytes - 1) == _lib.FW_EINVAL
    buf[2] = 5
    assert L.fw_chains_write_resample(a._h, _lib.RESAMPLE_FAMILY, ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    # a valid call still works afterwards, and a ladder may be set on a handle that has cloned
    a.clone([0, 0, 2, 3, 2])
    assert a.last_sources().tolist() == [0, 0, 2, 3, 2]
    lad = make("grid12_k4_pairs", 8, {}, monkeypatch)
    lad.clone(np.zeros(8, np.int32))
    lad.set_ladder([0.5, 0.7])
    assert code(lad.clone, np.arange(8)) == _lib.FW_EUNSUPPORTED
    assert code(lad.resample, 1.0, 1.5) == _lib.FW_EUNSUPPORTED
    maps = make("grid11x13_k4", 5, {}, monkeypatch)
    maps.enable_maps()
    assert code(maps.clone, np.arange(5)) == _lib.FW_ESTATE
    assert code(maps.resample, 1.0, 1.5) == _lib.FW_ESTATE


def test_checkpoint_across_a_resample(gpu_lib, monkeypatch):
    a = make("grid40_k4", 77, {}, monkeypatch)
    a.run(200)
    ref = resample_and_check(a, 0.5, 0.65, round=0)
    a.run(100)
    ck = a.checkpoint()
    assert np.array_equal(ck["families"], ref["src"])
    b = make("grid40_k4", 77)
    b.restore(ck)
    assert np.array_equal(b.families(), a.families())
    ia, ib = a.resample_info(), b.resample_info()
    assert (ib["n_resampled"], ib["clones"]) == (ia["n_resampled"], ia["clones"]) == (1, 77 - ref["survivors"])
    assert b.resample_round == a.resample_round == 1
    for ch in (a, b):
        ch.run(100)
    assert_same(a, b)
    # the next resample takes the same round and, from the same stats, draws the same map
    for ch in (a, b):
        ch.resample(0.65, 0.8)
    assert np.array_equal(a.last_sources(), b.last_sources())
    assert np.array_equal(a.families(), b.families())


def test_annealed_population_matches_a_direct_run_at_the_target_base(gpu_lib, monkeypatch):
    """The direction and scale of the weights: 10x10, k = 2; 8 handles x 512 chains of different
    seeds annealed base 1.0 -> 2.0 in 8 stages of 200 steps, against 4,096 chains run at base 2.0
    for the same 1,600 steps from the same seed plan.  The annealed side's SE is taken over the 8
    handle means; the means of the final cut agree within 4 combined SE.  (A sign or table error
    moves the mean by tens of SE: the base-1.0 and base-2.0 means are that far apart.)"""
    bases = np.geomspace(1.0, 2.0, 8)
    means, log_z = [], []
    for h in range(8):
        ch = make("grid10_k2_bi", 512, {}, monkeypatch, seed=1000 + h, base=1.0)
        out = ch.run_annealed(bases, 200)
        assert len(out["ess"]) == 7 and (out["ess"] > 1).all() and (out["ess"] <= 512 * 1.0001).all()
        assert ch.resample_info()["n_resampled"] == 7
        means.append(float(ch.stats()["cut"].mean()))
        log_z.append(out["log_z"])
    direct = make("grid10_k2_bi", 4096, {}, monkeypatch, seed=2000, base=2.0)
    direct.run(1600)
    cut = direct.stats()["cut"].astype(np.float64)
    hot = make("grid10_k2_bi", 512, {}, monkeypatch, seed=3000, base=1.0)
    hot.run(1600)
    m_a, se_a = float(np.mean(means)), float(np.std(means, ddof=1) / np.sqrt(8))
    m_d, se_d = float(cut.mean()), float(cut.std(ddof=1) / np.sqrt(len(cut)))
    se = float(np.hypot(se_a, se_d))
    m_hot = float(hot.stats()["cut"].mean())
    print(f"annealed {m_a:.4f} +- {se_a:.4f}  direct {m_d:.4f} +- {se_d:.4f}  "
          f"difference {m_a - m_d:+.4f} = {(m_a - m_d) / se:+.2f} combined SE; base 1.0 mean "
          f"{m_hot:.4f} ({(m_hot - m_d) / se:+.1f} SE away); log Z(2)/Z(1) {np.mean(log_z):.4f} "
          f"+- {np.std(log_z, ddof=1) / np.sqrt(8):.4f}")
    assert abs(m_hot - m_d) > 20 * se  # the test can tell the two bases apart
    assert abs(m_a - m_d) <= 4 * se
