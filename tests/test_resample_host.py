"""Properties of systematic resampling by cut as resample_ref.py restates it, of
population.weight_table and log_weight_mean (no GPU), and the limb arithmetic of the points
(csrc/fw_resample_limbs.h) against unsigned __int128 in a stand-alone host program
(tests/resample_div_check.cpp), built plainly and once more under the host compiler's address and
undefined-behaviour sanitizers."""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_ref
from flipcomplexityempirical_amd import population

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 30


def populations():
    """(name, cut, q, sign, u): random populations under both signs, steep and flat tables."""
    rng = np.random.default_rng(11)
    out = []
    for C, E, bases in ((1, 40, (1.0, 2.0)), (5, 40, (1.0, 1.3)), (77, 220, (2.0, 1.0)),
                        (77, 220, (1.0, 60.0)), (1024, 220, (1.0, 1.1)), (1500, 3120, (1.2, 1.0)),
                        (333, 64, (1.0, 1.0))):
        q, sign = population.weight_table(*bases, E)
        lo = int(rng.integers(0, E // 2))
        cut = rng.integers(lo, min(E, lo + 30) + 1, C)
        for u in (0, 0xFFFFFFFF, int(rng.integers(0, 2**32))):
            out.append((f"C{C}-b{bases[0]}to{bases[1]}-u{u}", cut, q, sign, u))
    return out


POPULATIONS = populations()


@pytest.mark.parametrize("name,cut,q,sign,u", POPULATIONS, ids=[p[0] for p in POPULATIONS])
def test_systematic_resampling_properties(name, cut, q, sign, u):
    C = len(cut)
    r = resample_ref.resample_map(cut, q, sign, u)
    n, W, T, src = r["offspring"], r["W"].astype(object), r["T"], r["src"]
    assert int(n.sum()) == C
    assert int(W.sum()) == T and int(W.max()) == ONE and T <= C * ONE
    assert r["S2"] == sum((int(w) >> 10) ** 2 for w in W)
    assert r["cref"] == (int(cut.min()) if sign == 1 else int(cut.max()))
    for i in range(C):  # the systematic-resampling bound
        x = Fraction(C * int(W[i]), T)
        assert math.floor(x) <= n[i] <= math.ceil(x), (i, x, n[i])
    # the map is idempotent and realises the offspring counts; survivors keep themselves
    assert np.array_equal(src[src], src)
    assert np.array_equal(np.bincount(src, minlength=C), n)
    assert np.array_equal(src[n > 0], np.flatnonzero(n > 0))
    assert r["survivors"] == int((n > 0).sum()) and r["max_offspring"] == int(n.max())
    # dead chains in ascending index take the extras in ascending survivor index
    assert (np.diff(src[n == 0]) >= 0).all()


def test_flat_table_gives_equal_weights_and_the_identity():
    q, sign = population.weight_table(1.5, 1.5, 100)
    assert (q == ONE).all()
    cut = np.random.default_rng(2).integers(0, 101, 200)
    for s in (sign, -sign):
        r = resample_ref.resample_map(cut, q, s, 12345)
        assert (r["W"] == ONE).all() and r["T"] == 200 * ONE
        assert np.array_equal(r["offspring"], np.ones(200, np.int64))
        assert np.array_equal(r["src"], np.arange(200))


def test_single_heavy_chain_and_one_chain():
    q, sign = population.weight_table(1.0, 1e9, 50)  # rho = 1e-9: q[1] = 1, q[2:] = 0
    assert sign == 1 and q[1] == 1 and not q[2:].any()
    cut = np.full(64, 30)
    cut[17] = 20
    r = resample_ref.resample_map(cut, q, sign, 999)
    assert r["T"] == ONE and r["survivors"] == 1 and r["max_offspring"] == 64
    assert (r["src"] == 17).all()
    one = resample_ref.resample_map([7], q, sign, 0xFFFFFFFF)
    assert one["src"].tolist() == [0] and one["offspring"].tolist() == [1] and one["T"] == ONE
    assert one["cref"] == 7


def test_weight_table_is_monotone_and_handles_both_signs():
    up, s_up = population.weight_table(1.0, 2.0, 300)
    down, s_down = population.weight_table(2.0, 1.0, 300)
    assert (s_up, s_down) == (1, -1)
    assert np.array_equal(up, down) and up.dtype == np.uint32
    assert up[0] == ONE and up[1] == ONE // 2 and up[30] == 1 and not up[32:].any()
    assert (np.diff(up.astype(np.int64)) <= 0).all()
    mu, s = population.weight_table(1.0, 2.63815853, 19800)
    assert s == 1 and len(mu) == 19801 and (np.diff(mu.astype(np.int64)) <= 0).all()
    assert mu[1] == round(ONE / 2.63815853)
    with pytest.raises(ValueError):
        population.weight_table(0.0, 1.0, 10)
    # the weight is r ** (-cut) under both signs: the lighter of two chains is the same one
    cut = np.array([10, 14])
    for b0, b1, heavy in ((1.0, 2.0, 0), (2.0, 1.0, 1)):
        q, sign = population.weight_table(b0, b1, 40)
        W = resample_ref.resample_map(cut, q, sign, 0)["W"]
        assert W[heavy] == ONE and W[1 - heavy] == round(ONE * 0.5 ** 4)


@pytest.mark.parametrize("b0,b1", [(1.0, 1.25), (1.25, 1.0), (0.8, 1.1)])
def test_log_weight_mean_agrees_with_floats(b0, b1):
    """Cuts within 10 of each other at ratio <= 1.375: every weight is above 2^25, so rounding
    to integers moves the mean by less than 2^-26 relative."""
    rng = np.random.default_rng(5)
    cut = rng.integers(100, 111, 500)
    q, sign = population.weight_table(b0, b1, 400)
    r = resample_ref.resample_map(cut, q, sign, 77)
    assert int(r["W"].min()) > 1 << 25
    info = {"T": r["T"], "S2": r["S2"], "cref": r["cref"]}
    got = population.log_weight_mean(info, b0, b1, len(cut))
    want = math.log(np.mean((b1 / b0) ** (-cut.astype(np.float64))))
    assert abs(got - want) <= 1e-9 * abs(want)
    raw = [0, 0, r["T"], r["S2"], r["cref"], 0, 0, 0]  # the int64 [8] form
    assert population.log_weight_mean(raw, b0, b1, len(cut)) == got
    w = r["W"].astype(np.float64)
    ess = population.effective_sample_size(info)
    assert abs(ess - w.sum() ** 2 / (w ** 2).sum()) <= 1e-4 * ess  # (w >> 10) drops 2^-15 of a weight above 2^25
    assert np.array_equal(population.family_sizes([0, 0, 2, 0]), [3, 0, 1, 0])


# ---------------------------------------------------------------- the points' limb arithmetic
def _build_and_run(tmp_path_factory, name, extra):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp(name) / "resample_div_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", *extra,
                    os.path.join(ROOT, "tests", "resample_div_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _check(out):
    for name, at_least in (("random", 10**6), ("extreme", 10**4), ("ascending", 10**5)):
        m = re.search(rf"^{name} cases (\d+) mismatches (\d+)$", out, re.M)
        assert m, (name, out)
        assert int(m.group(2)) == 0 and int(m.group(1)) >= at_least


def test_points_equal_int128(tmp_path_factory):
    _check(_build_and_run(tmp_path_factory, "rsm_div", []))


def test_points_equal_int128_under_sanitizers(tmp_path_factory):
    """A stand-alone program: the sanitizer runtimes are linked into it."""
    _check(_build_and_run(tmp_path_factory, "rsm_div_san",
                          ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_reference_points_equal_the_header_formula():
    """resample_ref.points is the formula itself; spot values computed by hand."""
    assert resample_ref.points(0, 4 * ONE, 4) == [0, ONE, 2 * ONE, 3 * ONE]
    assert resample_ref.points(0xFFFFFFFF, 4 * ONE, 4) == [ONE - 1, 2 * ONE - 1, 3 * ONE - 1,
                                                           4 * ONE - 1]
    assert resample_ref.points(1 << 31, 3, 2) == [0, 2]
