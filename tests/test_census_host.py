"""The ensemble census without a GPU: the entry points validate before they touch the device and
are bound; census_ref.py against a loop over chains and nodes; ensemble.py; and the kernel's
integer arithmetic (csrc/fw_census_plan.h) compiled by the host compiler
(tests/census_plan_check.cpp), as test_overlap_bits_host.py does for the overlap's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import census_ref
from flipcomplexityempirical_amd import _lib, ensemble
from flipcomplexityempirical_amd.graph import Graph, grid_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fw_chains_enable_census", "fw_chains_census_async", "fw_chains_read_census",
         "fw_chains_write_census", "fw_chains_census_reset", "fw_chains_census_info")


def test_symbols_are_bound_and_validate_before_the_device():
    L = _lib.load()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert set(NAMES) <= bound
    for name in NAMES:
        assert hasattr(L, name)
    assert L.fw_version() == 0x000700
    assert re.search(r" cen=[0-9a-f]{16}", _lib.build_info())
    # a bad mask is refused whatever the handle, a null handle whatever the mask
    for bad in (0, 8, 15, -1):
        assert L.fw_chains_enable_census(None, bad) == _lib.FW_EINVAL
        assert "mask" in L.fw_last_error().decode()
    for good in (1, 2, 4, 7):
        assert L.fw_chains_enable_census(None, good) == _lib.FW_EINVAL
        assert "null" in L.fw_last_error().decode()
    buf = np.zeros(4, np.uint64)
    info = np.zeros(5, np.int64)
    assert L.fw_chains_census_async(None) == _lib.FW_EINVAL
    assert L.fw_chains_read_census(None, _lib.CENSUS_OCC, _lib.ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_write_census(None, _lib.CENSUS_OCC, _lib.ptr(buf), buf.nbytes) == _lib.FW_EINVAL
    assert L.fw_chains_census_reset(None) == _lib.FW_EINVAL
    assert L.fw_chains_census_info(None, _lib.ptr(info)) == _lib.FW_EINVAL
    assert (_lib.CENSUS_NODES, _lib.CENSUS_EDGES, _lib.CENSUS_BOUNDARY) == (1, 2, 4)


def random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    adj = {v: set() for v in range(n)}
    for v in range(1, n):  # a spanning tree first, then extra edges
        u = int(rng.integers(0, v))
        adj[v].add(u), adj[u].add(v)
    while sum(len(a) for a in adj.values()) < 2 * m:
        u, v = (int(x) for x in rng.integers(0, n, 2))
        if u != v:
            adj[v].add(u), adj[u].add(v)
    return Graph.from_adjacency(list(range(n)), {v: sorted(a) for v, a in adj.items()})


@pytest.mark.parametrize("which", ["grid5x4", "random12"])
def test_census_ref_equals_a_loop(which):
    g = grid_graph(5, 4) if which == "grid5x4" else random_graph(12, 20, 3)
    rng = np.random.default_rng(11)
    k, C = 3, 14
    labels = rng.integers(0, k, (C, g.n)).astype(np.int16)
    labels[0] = 1  # a plan without a boundary
    for rungs, groups in ((None, 1), (rng.integers(0, 4, C), 4)):
        fast = census_ref.census(g, labels, k, rungs, groups)
        slow = census_ref.census_loop(g, labels, k, rungs, groups)
        for key in ("cnt", "occ", "ecut", "bnd"):
            assert fast[key].dtype == np.uint64 and fast[key].shape == slow[key].shape
            assert np.array_equal(fast[key], slow[key]), key
        assert fast["ecut"].shape[1] == g.n_edges
        assert int(fast["cnt"].sum()) == C
    twice = census_ref.add(census_ref.add(None, fast), fast)
    assert np.array_equal(twice["occ"], 2 * fast["occ"])


def test_ensemble_frequencies_entropy_and_part_sum():
    rng = np.random.default_rng(5)
    G, n, k = 2, 20, 4
    lab = rng.integers(0, k, (G, 30, n))
    occ = np.stack([[np.bincount(lab[g, :, v], minlength=k) for v in range(n)]
                    for g in range(G)]).astype(np.uint64)
    cnt = np.array([30, 30], np.uint64)
    f = ensemble.occupancy_frequency(occ, cnt)
    assert f.shape == (G, n, k) and np.allclose(f.sum(axis=2), 1.0)
    assert np.allclose(ensemble.occupancy_frequency(occ[1], cnt[1]), f[1])
    # entropy: 0 on a one-hot map, log k on a uniform one
    onehot = np.zeros((1, n, k), np.uint64)
    onehot[0, np.arange(n), np.arange(n) % k] = 7
    assert np.array_equal(ensemble.occupancy_entropy(onehot, [7]), np.zeros((1, n)))
    uniform = np.full((1, n, k), 5, np.uint64)
    assert np.allclose(ensemble.occupancy_entropy(uniform, [20]), np.log(k))
    # part_sum against the literal sum, default values and the reference's {-1, 1}
    lv = np.array([-1, 1, 5, -3])
    want = np.zeros((G, n), np.int64)
    for g in range(G):
        for v in range(n):
            for d in range(k):
                want[g, v] += int(lv[d]) * int(occ[g, v, d])
    assert np.array_equal(ensemble.part_sum_map(occ, lv), want)
    assert np.array_equal(ensemble.part_sum_map(occ), (lab.sum(axis=1)))
    with pytest.raises(ValueError):
        ensemble.part_sum_map(occ, [1, 2])
    ecut = rng.integers(0, 31, (G, 7)).astype(np.uint64)
    assert np.allclose(ensemble.edge_cut_frequency(ecut, cnt), ecut / 30.0)
    assert np.allclose(ensemble.boundary_frequency(ecut, cnt), ecut / 30.0)
    ecut[0] = 0  # a group nothing was counted in
    assert np.isnan(ensemble.edge_cut_frequency(ecut, [0, 30])[0]).all()


def test_symmetry_deviation_and_grid_images():
    h, w, k = 4, 4, 3
    perms = ensemble.grid_symmetries(h, w)
    assert perms.shape == (8, 16) and np.array_equal(perms[0], np.arange(16))
    assert len({tuple(p) for p in perms}) == 8
    assert ensemble.grid_symmetries(3, 5).shape == (4, 15)
    rng = np.random.default_rng(9)
    occ = rng.integers(1, 50, (1, h * w, k)).astype(np.uint64)
    cnt = np.array([100], np.uint64)
    assert ensemble.symmetry_deviation(occ, cnt, perms) > 0
    sym = sum(occ[:, p, :] for p in perms)  # invariant under the group
    assert ensemble.symmetry_deviation(sym, 8 * cnt, perms) < 1e-15
    # with a relabelling: swapping districts 0 and 1 under the left-right flip
    flip = perms[2]
    both = occ + occ[:, flip, :][..., [1, 0, 2]]
    assert ensemble.symmetry_deviation(both, 2 * cnt, [perms[0], flip],
                                       [[0, 1, 2], [1, 0, 2]]) < 1e-15
    # images: node (i, j) -> [i, j]; edge ids run node by node, right before below
    g = grid_graph(3, 5)
    img = ensemble.node_image(np.arange(15), 3, 5)
    assert img.shape == (3, 5) and img[2, 1] == 11
    e = g.edges()
    horiz, vert = ensemble.edge_images(np.arange(len(e)), 3, 5)
    assert horiz.shape == (3, 4) and vert.shape == (2, 5)
    for i in range(3):
        for j in range(5):
            if j < 4:
                assert tuple(e[horiz[i, j]]) == (i * 5 + j, i * 5 + j + 1)
            if i < 2:
                assert tuple(e[vert[i, j]]) == (i * 5 + j, (i + 1) * 5 + j)
    stacked = ensemble.edge_images(np.zeros((2, len(e))), 3, 5)
    assert stacked[0].shape == (2, 3, 4) and stacked[1].shape == (2, 2, 5)
    with pytest.raises(ValueError):
        ensemble.node_image(np.arange(14), 3, 5)


@pytest.fixture(scope="module")
def plan_check_output(tmp_path_factory):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("census_plan") / "census_plan_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "census_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("name,at_least", [
    ("field2", 10**5), ("field3", 10**5), ("field4", 10**5), ("field5", 10**5), ("field8", 10**5),
    ("straddle3", 10**4), ("straddle5", 10**4), ("reach", 1000), ("slices", 20000)])
def test_plan_header_equals_bitwise_loops(plan_check_output, name, at_least):
    m = re.search(rf"^{name} cases (\d+) mismatches (\d+)$", plan_check_output, re.M)
    assert m, (name, plan_check_output)
    assert int(m.group(2)) == 0
    assert int(m.group(1)) >= at_least
