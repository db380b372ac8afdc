"""Host side of the plan overlap (no GPU): the numpy reference the GPU tests compare with,
plandist.py, and the seven entry points' export and null-handle refusal."""
import itertools

import numpy as np
import pytest

import overlap_ref
from flipcomplexityempirical_amd import _lib, plandist

SYMBOLS = ("fw_chains_set_reference", "fw_chains_set_partners", "fw_chains_overlap_async",
           "fw_chains_read_overlap", "fw_chains_write_overlap", "fw_chains_overlap_reset",
           "fw_chains_overlap_info")


def plan_pair(seed=3, h=7, w=9, k=3, chains=4):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, k, (chains, h * w)).astype(np.int16)
    cur = ref.copy()
    flip = rng.random(cur.shape) < 0.3
    cur[flip] = rng.integers(0, k, int(flip.sum()))
    return ref, cur, k


def test_reference_equals_a_double_loop():
    ref, cur, k = plan_pair()
    O, dist = overlap_ref.overlap(ref, cur, k)
    for c in range(len(cur)):
        want = [[0] * k for _ in range(k)]
        differ = 0
        for v in range(cur.shape[1]):
            want[int(ref[c, v])][int(cur[c, v])] += 1
            differ += int(ref[c, v] != cur[c, v])
        assert O[c].tolist() == want
        assert int(dist[c]) == differ
    assert O.dtype == np.int64 and dist.dtype == np.int32
    # a shared reference is one row for every chain
    Os, ds = overlap_ref.overlap(ref[0], cur, k)
    assert np.array_equal(Os[0], O[0]) and ds[0] == dist[0]
    assert np.array_equal(Os[2], overlap_ref.overlap(np.tile(ref[0], (4, 1)), cur, k)[0][2])
    H = overlap_ref.dist_hist(dist, 63, groups=[0, 1, 1, 0], n_groups=2)
    assert H.shape == (2, 64) and H.dtype == np.uint64 and int(H.sum()) == 4
    assert H[0, dist[0]] >= 1 and H[1, dist[1]] >= 1
    assert np.array_equal(overlap_ref.dist_hist(dist, 63).sum(axis=0), H.sum(axis=0))


def test_hamming_and_retention():
    ref, cur, k = plan_pair()
    O, dist = overlap_ref.overlap(ref, cur, k)
    assert np.array_equal(plandist.hamming(O), dist.astype(np.float64))
    ret = plandist.retention(O)
    for c in range(len(cur)):
        for d in range(k):
            assert ret[c, d] == np.mean(cur[c][ref[c] == d] == d)
    empty = np.array([[3, 1], [0, 0]])
    r = plandist.retention(empty)
    assert r[0] == 0.75 and np.isnan(r[1])
    with pytest.raises(ValueError):
        plandist.hamming(np.zeros((2, 3)))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_matched_distance_equals_brute_force(k):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(k)
    O = rng.integers(0, 50, (6, k, k))
    # a relabelled copy of a plan is at matched distance 0
    O[0] = np.diag(rng.integers(1, 50, k))[:, rng.permutation(k)]
    got = plandist.matched_distance(O)
    for i in range(len(O)):
        best = max(sum(O[i, d, p[d]] for d in range(k)) for p in itertools.permutations(range(k)))
        assert got[i] == O[i].sum() - best
    assert got[0] == 0
    assert plandist.matched_distance(O[1]).shape == ()


def test_variation_of_information():
    same = np.diag([5, 7, 9])
    assert plandist.variation_of_information(same) == 0.0
    assert plandist.variation_of_information(same[:, [2, 0, 1]]) == 0.0  # names do not matter
    # independent uniform labellings of 4 nodes over 2 districts: H(R|X) + H(X|R) = 2 ln 2
    assert plandist.variation_of_information(np.ones((2, 2))) == pytest.approx(2 * np.log(2))
    # against the definition on a random table
    rng = np.random.default_rng(0)
    O = rng.integers(1, 30, (3, 4, 4))
    p = O / O.sum(axis=(1, 2), keepdims=True)
    h = lambda q: -(q * np.log(q)).sum()
    for i in range(3):
        want = 2 * h(p[i]) - h(p[i].sum(axis=0)) - h(p[i].sum(axis=1))
        assert plandist.variation_of_information(O)[i] == pytest.approx(want, rel=1e-12)


def test_distance_distribution():
    hist = np.zeros((2, 11), np.uint64)
    hist[0, 2], hist[0, 4] = 3, 1
    d = plandist.distance_distribution(hist)
    assert d["count"].tolist() == [4.0, 0.0]
    assert d["mean"][0] == 2.5 and d["std"][0] == pytest.approx(np.std([2, 2, 2, 4]))
    assert d["pmf"][0, 2] == 0.75 and np.isnan(d["pmf"][1]).all()
    assert plandist.distance_distribution(hist[0])["mean"].shape == (1,)


def test_overlap_symbols_exported_and_reject_null():
    L = _lib.load()
    assert {name for name, _, _ in _lib.SIGNATURES} >= set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    buf = np.zeros(8, np.int64)
    assert L.fw_chains_set_reference(None, None, 0) == _lib.FW_EINVAL
    assert L.fw_chains_set_partners(None, _lib.ptr(buf)) == _lib.FW_EINVAL
    assert L.fw_chains_overlap_async(None, _lib.OVERLAP_REFERENCE) == _lib.FW_EINVAL
    assert L.fw_chains_read_overlap(None, _lib.OVERLAP_DIST, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_write_overlap(None, _lib.OVERLAP_HIST, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_overlap_reset(None) == _lib.FW_EINVAL
    assert L.fw_chains_overlap_info(None, _lib.ptr(buf)) == _lib.FW_EINVAL
    assert L.fw_last_error().decode()
