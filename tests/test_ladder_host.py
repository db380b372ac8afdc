"""Replica exchange across a base ladder, host side (CPU): the layout validation, the ABI
surface without a device, and the swap rule itself on the reference restatement."""
import math

import numpy as np
import pytest

from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import check_ladder_layout, ladder_layout
from ladder_ref import exchange_counter, exchange_ref


def test_default_layout_is_valid():
    s, r = ladder_layout(12, 4)
    assert s.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert r.tolist() == [0, 1, 2, 3] * 3
    s2, r2 = check_ladder_layout(12, 4, s, r)
    assert s2.dtype == np.int32 and r2.dtype == np.int32
    # any placement with one chain per (set, rung) passes
    c = np.arange(12)
    check_ladder_layout(12, 4, c % 3, (c // 3 + c % 3) % 4)


def test_layout_validation():
    s, r = ladder_layout(12, 4)
    dup = r.copy()
    dup[1] = 0  # (set 0, rung 0) twice, (set 0, rung 1) missing
    with pytest.raises(ValueError, match="exactly one"):
        check_ladder_layout(12, 4, s, dup)
    miss = s.copy()
    miss[3] = 1  # set 0 loses its rung 3 to set 1
    with pytest.raises(ValueError):
        check_ladder_layout(12, 4, miss, r)
    with pytest.raises(ValueError, match="multiple"):
        check_ladder_layout(10, 4, *ladder_layout(10, 4))
    with pytest.raises(ValueError):
        check_ladder_layout(12, 4, s + 1, r)  # set id 3 of 3 sets
    with pytest.raises(ValueError):
        check_ladder_layout(12, 4, s, r - 1)
    with pytest.raises(ValueError):
        check_ladder_layout(2, 1, [0, 1], [0, 0])
    with pytest.raises(ValueError):
        check_ladder_layout(130, 65, *ladder_layout(130, 65))
    with pytest.raises(ValueError):
        check_ladder_layout(12, 4, s[:8], r[:8])


def test_rung_stats_record_is_64_bytes():
    assert _lib.RUNG_STATS_DTYPE.itemsize == 64
    assert _lib.RUNG_STATS_DTYPE.names == ("yields", "steps", "accepts", "sum_cut", "sum_bnodes",
                                           "sum_invb", "swap_tried", "swap_done")
    assert (_lib.READ_RUNG, _lib.READ_RUNG_STATS) == (8, 9)


def test_ladder_symbols_exported_and_reject_null():
    L = _lib.load()
    assert L.fw_chains_set_ladder(None, None, None, 2, None, None) == _lib.FW_EINVAL
    assert L.fw_last_error().decode()
    assert L.fw_chains_exchange_async(None, 0) == _lib.FW_EINVAL


def test_nonnegative_exponent_always_swaps():
    # x = d * (log b_r - log b_{r+1}) >= 0: the colder rung (larger base) holds the larger cut
    lb = [math.log(0.5), math.log(2.0)]
    for rnd in range(0, 400, 2):
        tried, done = exchange_ref([7, 9], [0, 0], lb, 11, rnd, 3)   # d < 0, lb[0] < lb[1]
        assert tried[0] and done[0]
        tried, done = exchange_ref([9, 9], [0, 0], lb, 11, rnd, 3)   # d = 0
        assert tried[0] and done[0]


def test_parity_and_stuck_chains_sit_out():
    lb = [0.0, 0.25, 0.5]
    tried, _ = exchange_ref([5, 5, 5], [0, 0, 0], lb, 1, 0, 0)
    assert tried.tolist() == [True, False, False]
    tried, _ = exchange_ref([5, 5, 5], [0, 0, 0], lb, 1, 1, 0)
    assert tried.tolist() == [False, True, False]  # the top rung has no rung above it
    tried, _ = exchange_ref([5, 5, 5], [0, 1, 0], lb, 1, 1, 0)
    assert not tried.any()


def test_swap_rate_matches_the_rule():
    """Fixed x = 2 * (-0.25) = -0.5 on both pairs of a 3-rung set: over 20,000 rounds (one pair
    tried per round) the swap rate lies within 4 binomial standard errors of e^x.  The draw is a
    function of the round, so the test is deterministic."""
    lb, cut, n = [0.0, 0.25, 0.5], [10, 8, 6], 20000
    done = 0
    for rnd in range(n):
        t, d = exchange_ref(cut, [0, 0, 0], lb, 2024, rnd, 17)
        assert t.sum() == 1
        done += int(d.sum())
    p = math.exp(-0.5)
    se = math.sqrt(p * (1 - p) / n)
    print(f"swap rate {done / n:.5f}, e^x {p:.5f}, 4 se {4 * se:.5f}")
    assert abs(done / n - p) <= 4 * se


def test_exchange_counters_are_disjoint_from_the_other_draws():
    # proposal draws: word 1 = hi32(t) < 2^30; wait draws: bit 31 set
    for r in (0, 1, 63):
        for rnd in (0, 5, 2 ** 32 - 1):
            c = exchange_counter(rnd, r, 17 + (5 << 32))
            assert c[1] >> 30 == 1, hex(c[1])
            assert c[0] == rnd and c[2] == 17 and c[3] == 5
            assert c[1] & 0x3FFFFFFF == r
