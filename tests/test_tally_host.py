"""Host side of the district tallies: the partisan scores of elections.py on hand-computed
plans, Graph.columns, the seat-histogram merge, the reference restatement itself, and the
argument checks of the tally entry points that need no device."""
import numpy as np
import pytest

import tally_ref
from flipcomplexityempirical_amd import _lib, elections
from flipcomplexityempirical_amd.distributed import merge_seat_hist
from flipcomplexityempirical_amd.graph import Graph, grid_graph


# one plan, four districts: A wins 60-40, ties 50-50, loses 20-80, sweeps 30-0
A = np.array([60, 50, 20, 30])
B = np.array([40, 50, 80, 0])


def test_scores_on_a_hand_computed_plan():
    shares = elections.vote_shares(A, B)
    assert shares.tolist() == [0.6, 0.5, 0.2, 1.0]
    assert int(elections.seats(A, B)) == 2  # the tied district is nobody's seat
    # median of {0.2, 0.5, 0.6, 1.0} = 0.55, mean = 0.575
    assert elections.mean_median(A, B) == pytest.approx(0.55 - 0.575, abs=1e-15)
    # wasted A: 60 - 50, 50 (a tie is not a win), 20, 30 - 15; wasted B: 40, 50 - 50, 80 - 50, 0
    wa, wb = 10 + 50 + 20 + 15, 40 + 0 + 30 + 0
    assert elections.efficiency_gap(A, B) == pytest.approx((wb - wa) / 330, abs=1e-15)


def test_all_a_sweep_and_empty_district():
    a, b = np.array([10, 20, 30]), np.array([0, 0, 0])
    assert int(elections.seats(a, b)) == 3
    assert elections.vote_shares(a, b).tolist() == [1.0, 1.0, 1.0]
    assert float(elections.mean_median(a, b)) == 0.0
    # A wastes half of every district, B nothing: (0 - 30) / 60
    assert float(elections.efficiency_gap(a, b)) == -0.5
    # a district without votes: its share is NaN and the share-based score propagates it; the
    # efficiency gap, which only adds votes up, does not
    a0, b0 = np.array([10, 0, 5]), np.array([5, 0, 10])
    sh = elections.vote_shares(a0, b0)
    assert np.isnan(sh[1]) and sh[0] == 10 / 15 and sh[2] == 5 / 15
    assert np.isnan(elections.mean_median(a0, b0))
    assert int(elections.seats(a0, b0)) == 1
    assert float(elections.efficiency_gap(a0, b0)) == pytest.approx(0.0, abs=1e-15)
    assert np.isnan(elections.efficiency_gap(np.zeros(3), np.zeros(3)))


def test_scores_are_vectorised_over_chains():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 50, (7, 5))
    b = rng.integers(0, 50, (7, 5))
    for f in (elections.seats, elections.mean_median, elections.efficiency_gap):
        got = f(a, b)
        assert got.shape == (7,)
        for i in range(7):
            assert np.array_equal(got[i], f(a[i], b[i]), equal_nan=True)
    assert elections.vote_shares(a, b).shape == (7, 5)
    with pytest.raises(ValueError):
        elections.seats(a, b[:, :4])


def test_seat_distribution_normalises_rows():
    h = np.array([[[1, 3, 0]], [[0, 0, 0]]], np.uint64)
    d = elections.seat_distribution(h)
    assert d[0, 0].tolist() == [0.25, 0.75, 0.0]
    assert np.isnan(d[1, 0]).all()


def test_graph_columns_casts_and_errors():
    g = grid_graph(2, 3)
    g.node_attrs = [{"TOTPOP": str(10 + x), "pink": x % 2, "area": 1.5, "half": 2.0}
                    for x in range(g.n)]
    cols = g.columns(["TOTPOP", "pink", "half"])
    assert cols.dtype == np.int64 and cols.shape == (3, 6)
    assert cols[0].tolist() == [10, 11, 12, 13, 14, 15]  # the TOTPOP str -> int cast
    assert cols[1].tolist() == [0, 1, 0, 1, 0, 1]
    assert cols[2].tolist() == [2] * 6
    with pytest.raises(ValueError, match="no attribute"):
        g.columns(["purple"])
    with pytest.raises(ValueError, match="not an integer"):
        g.columns(["area"])
    g.node_attrs[4]["TOTPOP"] = "12.5"
    with pytest.raises(ValueError, match="not an integer"):
        g.columns(["TOTPOP"])
    with pytest.raises(ValueError, match="no node attributes"):
        Graph(rowptr=g.rowptr, col=g.col).columns(["TOTPOP"])


def test_merge_seat_hist_at_world_one():
    h = np.arange(2 * 3 * 5, dtype=np.uint64).reshape(2, 3, 5) + np.uint64(2 ** 40)
    out = merge_seat_hist(h, None)
    assert out.dtype == np.uint64 and np.array_equal(out, h)


def test_reference_on_a_hand_computed_plan():
    """tally_ref against sums written out by hand: 6 nodes, 3 districts, one of them tied, one
    won by a single vote, one without votes."""
    labels = np.array([[0, 0, 1, 1, 2, 2], [2, 1, 0, 0, 1, 2]], np.int16)
    cols = np.array([[3, 4, 5, 1, 0, 0], [2, 5, 2, 3, 0, 0]])
    T, S, H = tally_ref.tally(labels, cols, 3, [(0, 1)])
    assert T[0].tolist() == [[7, 6, 0], [7, 5, 0]]  # tie, A by one, empty (a tie)
    assert S[0].tolist() == [[1, 2]]
    assert T[1].tolist() == [[6, 4, 3], [5, 5, 2]]
    assert S[1].tolist() == [[2, 0]]
    assert H.tolist() == [[[0, 1, 1, 0]]]
    H2 = tally_ref.seat_hist(S, 3, groups=[1, 0], n_groups=2)
    assert H2.tolist() == [[[0, 0, 1, 0]], [[0, 1, 0, 0]]]


def test_tally_entry_points_check_arguments_without_a_device():
    L = _lib.load()
    cols = np.ones((1, 4), np.int64)
    ab = np.array([[0, 1]], np.int32)
    info = np.zeros(5, np.int64)
    buf = np.zeros(8, np.int64)
    assert L.fw_chains_set_columns(None, _lib.ptr(cols), 1) == _lib.FW_EINVAL
    assert L.fw_last_error().decode()
    assert L.fw_chains_set_elections(None, _lib.ptr(ab), 1) == _lib.FW_EINVAL
    assert L.fw_chains_tally_async(None) == _lib.FW_EINVAL
    assert L.fw_chains_read_tally(None, _lib.TALLY_SUMS, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_write_tally(None, _lib.TALLY_HIST, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_tally_reset(None) == _lib.FW_EINVAL
    assert L.fw_chains_tally_info(None, _lib.ptr(info)) == _lib.FW_EINVAL
    assert (_lib.TALLY_SUMS, _lib.TALLY_SEATS, _lib.TALLY_HIST) == (0, 1, 2)
