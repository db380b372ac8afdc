"""Observable series on the GPU (fw_chains_enable_series .. fw_chains_series_acf): recording
against a handle driven stepwise, the by-rung view against the host permutation, the exact
lagged sums and the pooled autocovariances against series_ref.py bit for bit, the refusals,
and checkpoint / resume."""
import functools

import numpy as np
import pytest

import series_ref
from cases import cases
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.chain import Chains, DeviceGraph

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases(include_kansas=False)}
SEED, ID0, ROUND0, SAMPLES, STEPS = 2024, 17, 5, 40, 25
LADDER, PLAIN = "grid12_k4_pairs", "grid10_k2_bi"
N_RUNGS, N_SETS = 4, 3   # the ladder case: 12 chains
PLAIN_CHAINS = 70        # one full wave and a tail of 6


def scrambled_layout(n_rungs=N_RUNGS, n_sets=N_SETS):
    """As in test_gpu_ladder.py: sets interleaved, rungs rotated per set."""
    c = np.arange(n_rungs * n_sets)
    s = c % n_sets
    return s.astype(np.int32), ((c // n_sets + s) % n_rungs).astype(np.int32)


def ladder_bases(n_rungs=N_RUNGS):
    return np.geomspace(0.5, 2.0, n_rungs)  # test_gpu_ladder.py: swaps do happen


def make(name, n_chains=None, ladder=None, seed=SEED):
    case = CASES[name]
    ladder = name == LADDER if ladder is None else ladder
    if n_chains is None:
        n_chains = N_RUNGS * N_SETS if ladder else PLAIN_CHAINS
    ch = Chains(DeviceGraph(case.graph), n_chains, case.k, case.init, proposal=case.mode,
                pop_bounds=case.bounds, base=case.base, seed=seed, chain_id0=ID0)
    if ladder:
        ch.set_ladder(ladder_bases(), *scrambled_layout())
    return ch


def xmax_of(name):
    g = CASES[name].graph
    return max(len(g.col) // 2, g.n)


def recorded(name, n_samples=SAMPLES):
    """A handle with ``n_samples`` samples recorded STEPS steps apart."""
    ch = make(name)
    ch.enable_series(SAMPLES)
    if name == LADDER:
        ch.run_tempered(STEPS, n_samples, round0=ROUND0, record=True)
    else:
        ch.run_sampled(STEPS, n_samples)
    return ch


@functools.lru_cache(maxsize=None)
def shared(name):
    """One recorded handle per case for the tests that only read it."""
    return recorded(name)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def assert_same_state(a, b):
    assert np.array_equal(a.labels(), b.labels())
    sa, sb = a.stats(), b.stats()
    for f in sa.dtype.names:
        x, y = sa[f], sb[f]
        if f == "sum_invb":
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f
    assert np.array_equal(a.hist_cut(), b.hist_cut()) and np.array_equal(a.hist_b(), b.hist_b())


def refused(code, fn, *args, **kw):
    with pytest.raises(_lib.FlipwalkError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    assert _lib.load().fw_last_error().decode()


# ------------------------------------------------------------------ recording
@pytest.mark.parametrize("kernel_path", ["auto", "wave64"])
@pytest.mark.parametrize("name", [LADDER, PLAIN])
def test_recording_equals_stepwise(gpu_lib, name, kernel_path, monkeypatch):
    """40 samples x 25 steps enqueued back to back (run_tempered(record=True) on the 12-chain
    ladder, run_sampled on 70 plain chains) against a second handle, without series, driven
    by blocking calls: its stats()["cut"], stats()["bnodes"] and rungs(), read after each run
    and before the exchange, are the series rows; and both handles end in the same state."""
    if kernel_path == "wave64":
        monkeypatch.setenv("FLIPWALK_NO_GRID16", "1")
    else:
        monkeypatch.delenv("FLIPWALK_NO_GRID16", raising=False)
    a = recorded(name)
    info = a.series_info()
    assert (info["capacity"], info["n_samples"]) == (SAMPLES, SAMPLES)
    b = make(name)
    cut, bn, rung = [], [], []
    for i in range(SAMPLES):
        b.run(STEPS)
        st = b.stats()
        cut.append(st["cut"].copy())
        bn.append(st["bnodes"].copy())
        if name == LADDER:
            rung.append(b.rungs())
            b.exchange(ROUND0 + i)
        else:
            rung.append(np.full(b.n_chains, -1, np.int32))
    b.sync()
    assert np.array_equal(a.series("cut"), np.stack(cut))
    assert np.array_equal(a.series("bnodes"), np.stack(bn))
    assert np.array_equal(a.series("rung"), np.stack(rung))
    assert a.series("cut").dtype == np.int32 and a.series("cut").shape == (SAMPLES, a.n_chains)
    # recording perturbed nothing
    assert_same_state(a, b)
    if name == LADDER:
        assert np.array_equal(a.rungs(), b.rungs())
        assert a.ladder_round == ROUND0 + SAMPLES
    # a window
    assert np.array_equal(a.series("bnodes", t0=3, n=30), np.stack(bn)[3:33])
    # reset_observables leaves the series alone; series_reset empties them
    a.reset_observables()
    assert a.n_samples == SAMPLES and np.array_equal(a.series("cut"), np.stack(cut))
    a.series_reset()
    assert a.n_samples == 0 and a.series("cut").shape == (0, a.n_chains)


def test_by_rung_view(gpu_lib):
    ch = shared(LADDER)
    s, _ = scrambled_layout()
    rung = ch.series("rung")
    slots = s[None, :].astype(np.int64) * N_RUNGS + rung
    assert (np.sort(slots, axis=1) == np.arange(ch.n_chains)[None, :]).all()
    # at least one swap: the view is not one fixed permutation
    assert (rung != rung[0]).any()
    for what in ("cut", "bnodes"):
        want = series_ref.regroup(ch.series(what), rung, s, N_RUNGS)
        assert np.array_equal(ch.series(what, by_rung=True), want), what
        assert np.array_equal(ch.series(what, by_rung=True, t0=3, n=30), want[3:33]), what


# ------------------------------------------------------------------ lagged sums, pooled
def check_acf(ch, what, max_lag, x, by_rung=False, t0=0, n=None):
    """per_series exactly and pooled bitwise against series_ref on the host copy x."""
    pooled, sums = ch.series_acf(what, max_lag, by_rung=by_rung, t0=t0, n=n, per_series=True)
    want_sums, want_pooled = series_ref.series_acf(x, max_lag, N_RUNGS if by_rung else 0)
    assert sums.dtype == np.int64 and np.array_equal(sums, want_sums), (what, max_lag)
    assert pooled.shape == want_pooled.shape
    assert same_bits(pooled, want_pooled), (what, max_lag, pooled, want_pooled)
    # pooled alone (no per_series output) is the same
    assert same_bits(ch.series_acf(what, max_lag, by_rung=by_rung, t0=t0, n=n), want_pooled)


@pytest.mark.parametrize("name", [LADDER, PLAIN])
def test_acf_on_recorded_data(gpu_lib, name):
    ch = shared(name)
    for what in ("cut", "bnodes"):
        x = ch.series(what)
        for max_lag in (0, 17, 39):
            check_acf(ch, what, max_lag, x)
        check_acf(ch, what, 17, x[3:33], t0=3, n=30)
        check_acf(ch, what, 29, x[3:33], t0=3, n=30)
    if name == LADDER:  # three sets per group
        y = ch.series("cut", by_rung=True)
        for max_lag in (0, 17, 39):
            check_acf(ch, "cut", max_lag, y, by_rung=True)
        check_acf(ch, "cut", 17, y[3:33], by_rung=True, t0=3, n=30)


def synthetic(name, n_chains, n, seed):
    """A handle whose cut series holds chosen values: random in [0, xmax], series 0 constant,
    series 1 at xmax throughout."""
    xmax = xmax_of(name)
    x = np.random.default_rng(seed).integers(0, xmax + 1, (n, n_chains)).astype(np.int32)
    x[:, 0] = 97
    x[:, 1] = xmax
    ch = make(name, n_chains=n_chains, ladder=False)
    ch.enable_series(n)
    ch.write_series("cut", x)
    assert ch.n_samples == n and np.array_equal(ch.series("cut"), x)
    return ch, x


def test_acf_synthetic_130(gpu_lib):
    """130 series (two waves and a tail of 2) x 200 samples; lag counts that are not multiples
    of the 32-lag chunk, one past two chunks, and the longest the window allows."""
    ch, x = synthetic(PLAIN, 130, 200, 1)
    for max_lag in (37, 64, 199):
        check_acf(ch, "cut", max_lag, x)
    pooled = ch.series_acf("cut", 37)
    sums = series_ref.lagged_sums(x[:, :2], 37)
    # the constant series and the one at xmax have zero autocovariance, exactly
    assert not series_ref.terms(sums, 200)[:, :38].any()
    assert pooled[0, 0] > 0


def test_acf_lag_cap(gpu_lib):
    """max_lag = 1,023 (32 chunks of 32 lags) on 5 series of 1,100 samples; and past the cap."""
    ch, x = synthetic(PLAIN, 5, 1100, 2)
    check_acf(ch, "cut", _lib.SERIES_MAX_LAG, x)
    refused(_lib.FW_EINVAL, ch.series_acf, "cut", _lib.SERIES_MAX_LAG + 1)
    ch.series_acf("cut", 1023, t0=76, n=1024)
    refused(_lib.FW_EINVAL, ch.series_acf, "cut", 1023, t0=77, n=1023)  # max_lag >= n


def test_pooled_600(gpu_lib):
    """600 members: three rows of 256 partials, the last one ragged (88)."""
    ch, x = synthetic(PLAIN, 600, 50, 3)
    for max_lag in (0, 5):
        check_acf(ch, "cut", max_lag, x)


def test_by_rung_mean_is_the_integer_sum(gpu_lib):
    """The by-rung pooled sum of means is, to the last bit, the ordered sum over the sets of
    (integer sum of the slot's by-rung series) / n: no statistical threshold."""
    ch = shared(LADDER)
    y = ch.series("cut", by_rung=True).astype(np.int64)
    n = y.shape[0]
    m = y.sum(axis=0).astype(np.float64) / np.float64(n)
    pooled = ch.series_acf("cut", 0, by_rung=True)
    for r in range(N_RUNGS):
        want = series_ref.ordered_sum(m[r::N_RUNGS, None])
        assert same_bits(pooled[r, 1:2], want), r


# ------------------------------------------------------------------ refusals
def test_series_refusals(gpu_lib):
    E, S = _lib.FW_EINVAL, _lib.FW_ESTATE
    ch = make(LADDER)
    refused(S, ch.record)  # before enable
    refused(S, ch.series, "cut", 0, 0, 1)
    refused(E, ch.enable_series, 0)
    ch.enable_series(6)
    refused(S, ch.enable_series, 6)  # once
    ch.run(10)
    ch.record()
    ch.record()
    assert ch.n_samples == 2
    refused(E, ch.series, "cut", False, 1, 2)  # window past the recorded samples
    refused(E, ch.series, "cut", False, -1, 1)
    refused(E, ch.series_acf, "cut", 2)   # max_lag >= n
    refused(E, ch.series_acf, "cut", -1)
    refused(E, ch.series_acf, "rung", 0)
    refused(E, ch.series, "rung", True)   # by-rung applies to cut and bnodes
    # a new ladder: the two samples so far belong to the old one
    s, _ = scrambled_layout()
    ch.set_ladder(ladder_bases(), s, ch.rungs())
    ch.run(10)
    ch.record()
    ch.record()
    assert ch.series_info()["epoch"] == 2
    refused(S, ch.series, "cut", True)                 # window spans the set_ladder
    refused(S, ch.series_acf, "cut", 1, True)
    assert ch.series("cut", by_rung=True, t0=2, n=2).shape == (2, ch.n_chains)
    assert ch.series_acf("cut", 1, by_rung=True, t0=2, n=2).shape == (N_RUNGS, 4)
    # rung writes are validated: a (set, rung) held twice, a rung outside the ladder
    rows = ch.series("rung", t0=2, n=2)
    bad = rows.copy()
    bad[1, 0] = bad[1, N_SETS]  # chains 0 and N_SETS are in set 0
    refused(E, ch.write_series, "rung", bad, 2)
    bad = rows.copy()
    bad[0, 0] = N_RUNGS
    refused(E, ch.write_series, "rung", bad, 2)
    assert np.array_equal(ch.series("rung", t0=2, n=2), rows)  # refused writes wrote nothing
    ch.write_series("rung", ch.series("rung", t0=2, n=2)[::-1][:1], 0)  # stamps sample 0
    refused(S, ch.series, "cut", True, 0, 2)  # sample 1 still belongs to the old ladder
    assert ch.series("cut", by_rung=True, t0=0, n=1).shape == (1, ch.n_chains)
    # value writes: no gaps, inside the capacity, values in [0, xmax]
    ok = np.zeros((1, ch.n_chains), np.int32)
    refused(E, ch.write_series, "cut", ok, 5)
    refused(E, ch.write_series, "cut", np.zeros((3, ch.n_chains), np.int32), 4)
    refused(E, ch.write_series, "cut", ok - 1, 0)
    refused(E, ch.write_series, "cut", ok + xmax_of(LADDER) + 1, 0)
    ch.write_series("cut", ok, 4)
    ch.record()
    assert ch.n_samples == 6
    refused(S, ch.record)  # full
    ch.run(10)             # the handle still runs
    assert (ch.stats()["steps"] == 30).all()
    # by-rung without a ladder
    p = make(PLAIN, n_chains=8)
    p.enable_series(2)
    p.record()
    refused(S, p.series, "cut", True)
    refused(S, p.series_acf, "cut", 0, True)
    assert (p.series("rung") == -1).all()


# ------------------------------------------------------------------ checkpoint
def test_series_checkpoint_resume(gpu_lib, tmp_path):
    whole = shared(LADDER)
    half = SAMPLES // 2
    first = recorded(LADDER, half)
    path = str(tmp_path / "series.npz")
    first.save_checkpoint(path)
    case = CASES[LADDER]
    resumed = Chains.from_checkpoint(DeviceGraph(case.graph), path, case.k)
    assert resumed.series_info() == first.series_info() | {"epoch": 1}
    for what in ("cut", "bnodes", "rung"):
        assert np.array_equal(resumed.series(what), first.series(what)), what
    resumed.run_tempered(STEPS, SAMPLES - half, record=True)
    assert resumed.ladder_round == ROUND0 + SAMPLES
    assert_same_state(resumed, whole)
    for what in ("cut", "bnodes", "rung"):
        assert np.array_equal(resumed.series(what), whole.series(what)), what
    for by_rung in (False, True):
        assert np.array_equal(resumed.series("cut", by_rung=by_rung),
                              whole.series("cut", by_rung=by_rung))
        got = resumed.series_acf("cut", 17, by_rung=by_rung, per_series=True)
        want = whole.series_acf("cut", 17, by_rung=by_rung, per_series=True)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
