"""Host side of the per-district geometry (no GPU): compactness.py, Graph.edge_column, the
numpy reference the GPU tests compare with, and Chains.set_geometry's argument checks."""
import json
import math

import numpy as np
import pytest

import geometry_ref
from flipcomplexityempirical_amd import compactness as cp
from flipcomplexityempirical_amd.chain import check_geometry_arrays
from flipcomplexityempirical_amd.graph import Graph, block_seed, grid_graph


def test_quantise_rounds_and_refuses():
    q = cp.quantise([0.0, 1.26, 2.5, 3.49], 10)
    assert q.dtype == np.int64 and q.tolist() == [0, 13, 25, 35]  # rint: halves to even
    assert cp.quantise(np.array([3, 4])).tolist() == [3, 4]
    assert cp.quantise([2 ** 31 - 1]).tolist() == [2 ** 31 - 1]
    assert cp.quantise(np.zeros(0)).shape == (0,)
    for bad in ([1.0, -0.5], [np.nan], [np.inf], [2.0 ** 31], [2.0 ** 30, 2.0 ** 30]):
        with pytest.raises(ValueError):
            cp.quantise(bad)
    with pytest.raises(ValueError):
        cp.quantise([1.0, 2.0], 2.0 ** 31)  # the scaled total
    with pytest.raises(ValueError):
        cp.quantise([1.0], 0)


def block_geometry():
    """A 12 x 12 unit grid in four 6 x 6 blocks: unit edge weights, unit areas, exterior = a
    node's sides on the outer ring."""
    g = grid_graph(12, 12)
    lab = block_seed(12, 12, 2, 2)[None, :]
    i, j = np.divmod(np.arange(144), 12)
    ext = ((i == 0).astype(np.int64) + (i == 11) + (j == 0) + (j == 11))
    return g, lab, ext, geometry_ref.districts(lab, g.edges(), 4, exterior=ext)


def test_polsby_popper_of_a_square_block():
    g, lab, ext, G = block_geometry()
    assert G[0].tolist() == [[36, 12, 12, 12, 36]] * 4  # A = 36, P = 12 + 12 = 24
    assert np.array_equal(cp.perimeters(G), np.full((1, 4), 24.0))
    pp = cp.polsby_popper(G)
    assert pp.shape == (1, 4) and np.allclose(pp, 4 * math.pi * 36 / 24 ** 2, rtol=1e-15)
    # lengths quantised at 100 per unit, areas at 10: the scales take them back
    Gs = G * np.array([1, 1, 100, 100, 10])
    assert np.allclose(cp.polsby_popper(Gs, length_scale=100, area_scale=10), pp, rtol=1e-15)
    assert np.array_equal(cp.perimeters(Gs, 100), cp.perimeters(G))
    lone = np.array([[5, 0, 0, 0, 5], [1, 2, 3, 4, 5]])
    out = cp.polsby_popper(lone)
    assert np.isnan(out[0]) and out[1] == pytest.approx(4 * math.pi * 5 / 49)
    with pytest.raises(ValueError):
        cp.polsby_popper(np.zeros((4, 3)))


def test_cut_edge_share_sums_to_two():
    g = grid_graph(9, 7)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 5, (6, 63)).astype(np.int16)
    G = geometry_ref.districts(lab, g.edges(), 5)
    share = cp.cut_edge_share(G)
    assert share.shape == (6, 5) and np.allclose(share.sum(axis=1), 2.0, rtol=1e-15)
    assert np.isnan(cp.cut_edge_share(np.zeros((3, 5)))).all()  # a plan without a cut edge
    d = cp.district_cut_distribution(geometry_ref.cut_hist(G, g.n_edges))
    assert d.shape == (1, g.n_edges + 1) and d.sum() == pytest.approx(1.0)
    assert np.isnan(cp.district_cut_distribution(np.zeros((2, 4)))).all()


def small_networkx():
    import networkx as nx
    G = nx.Graph()
    for a, b, perim in (("c", "a", 2.5), ("a", "b", 1.25), ("b", "d", 0.0), ("d", "c", 7.0),
                        ("a", "d", 3.0)):
        G.add_edge(a, b, shared_perim=perim)
    return G


def test_edge_column_follows_edges_order(tmp_path):
    import networkx as nx
    G = small_networkx()
    g = Graph.from_networkx(G)
    assert g.nodes == ["a", "b", "c", "d"]
    pairs = [(g.nodes[u], g.nodes[w]) for u, w in g.edges()]
    assert pairs == [("a", "b"), ("a", "c"), ("a", "d"), ("b", "d"), ("c", "d")]
    want = [125, 250, 300, 0, 700]
    col = g.edge_column("shared_perim", 100)
    assert col.dtype == np.int64 and col.tolist() == want
    assert g.edge_column("shared_perim").tolist() == [1, 2, 3, 0, 7]
    with pytest.raises(ValueError):
        g.edge_column("length")
    path = tmp_path / "adj.json"
    path.write_text(json.dumps(nx.adjacency_data(G)))
    gj = Graph.from_json(str(path), pop_col=None)
    assert np.array_equal(gj.edges(), g.edges())
    assert gj.edge_column("shared_perim", 100).tolist() == want
    G.edges["a", "b"]["shared_perim"] = -1.0
    with pytest.raises(ValueError):
        Graph.from_networkx(G).edge_column("shared_perim")
    # the existing constructors keep their behaviour: no edge attributes unless given
    assert grid_graph(3, 3).edge_attrs is None
    assert Graph.from_adjacency([0, 1], {0: [1], 1: [0]}).edge_attrs is None
    with pytest.raises(ValueError):
        grid_graph(3, 3).edge_column("shared_perim")


def brute_force(lab, g, k, w, a, x):
    out = np.zeros((len(lab), k, 5), np.int64)
    for c, plan in enumerate(lab):
        for v in range(g.n):
            d = int(plan[v])
            out[c, d, 0] += 1
            out[c, d, 3] += int(x[v])
            out[c, d, 4] += int(a[v])
        for e, (u, v) in enumerate(g.edges()):
            if plan[u] != plan[v]:
                for d in (int(plan[u]), int(plan[v])):
                    out[c, d, 1] += 1
                    out[c, d, 2] += int(w[e])
    return out


def test_reference_against_a_python_loop():
    g = grid_graph(5, 4)
    rng = np.random.default_rng(11)
    lab = rng.integers(0, 3, (4, 20)).astype(np.int16)
    lab[3] = 1  # one district holds everything: no cut edge, two empty districts
    w = rng.integers(0, 1000, g.n_edges)
    a = rng.integers(0, 1000, 20)
    x = rng.integers(0, 1000, 20)
    G = geometry_ref.districts(lab, g.edges(), 3, w, a, x)
    assert G.dtype == np.int64 and np.array_equal(G, brute_force(lab, g, 3, w, a, x))
    ones, zeros = np.ones(g.n_edges, np.int64), np.zeros(20, np.int64)
    assert np.array_equal(geometry_ref.districts(lab, g.edges(), 3),
                          brute_force(lab, g, 3, ones, np.ones(20, np.int64), zeros))
    H = geometry_ref.cut_hist(G, g.n_edges, groups=[0, 1, 1, 0], n_groups=2)
    assert H.shape == (2, g.n_edges + 1) and H.dtype == np.uint64
    want = np.zeros_like(H)
    for c, grp in enumerate([0, 1, 1, 0]):
        for d in range(3):
            want[grp, G[c, d, 1]] += 1
    assert np.array_equal(H, want) and int(H[0, 0]) >= 3  # the uncut plan's three districts


def test_set_geometry_argument_checks():
    n, E = 20, 31
    ok = check_geometry_arrays(n, E, np.arange(E), None, np.ones(n, np.uint8))
    assert ok[1] is None and ok[0].dtype == ok[2].dtype == np.int64
    assert ok[0].flags["C_CONTIGUOUS"] and ok[0].tolist() == list(range(E))
    assert check_geometry_arrays(n, E) == (None, None, None)
    big = np.zeros(n, np.int64)
    big[3], big[7] = 2 ** 31 - 5, 4  # a total of 2^31 - 1 is allowed
    assert int(check_geometry_arrays(n, E, area=big)[1].sum()) == 2 ** 31 - 1
    big[7] = 5  # exactly 2^31
    neg = np.ones(n, np.int64)
    neg[4] = -1
    for kw in ({"edge_weights": np.ones(E)},              # floats
               {"area": np.ones(n, bool)},
               {"edge_weights": np.ones(n, np.int64)},    # a node-length array for the edges
               {"area": np.ones((n, 1), np.int64)},
               {"exterior": np.ones(E, np.int64)},
               {"exterior": neg},
               {"area": big},
               {"edge_weights": np.full(E, 2 ** 62, np.uint64)}):
        with pytest.raises(ValueError):
            check_geometry_arrays(n, E, **kw)
