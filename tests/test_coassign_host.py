"""The node co-assignment step without a GPU: the plan and bit arithmetic of
csrc/fw_coassign_plan.h on the host, the library's provenance and null-handle refusals, and the
numpy scores of flipcomplexityempirical_amd/coassign.py.

The header holds the arithmetic as plain functions on integers, so tests/coassign_plan_check.cpp
compiles the same text with the host compiler: for each label width and random label matrices
with 1..97 members the restated planes must equal the fields' bits with zero pad bits,
per_group - popcount(diff) must equal a per-member loop (pairs that differ in one bit included),
and the plan's tiles, windows and chunks must cover every entry and member word exactly once
inside the LDS bound.  The program is built plainly and once more under the host compiler's
address and undefined-behaviour sanitizers; it is a stand-alone program, so their runtimes are
linked into it.
"""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import coassign_ref
from flipcomplexityempirical_amd import _lib, coassign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 3, 4, 5, 8)


def _build_and_run(tmp_path_factory, name, extra):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp(name) / "coassign_plan_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *extra,
                    os.path.join(ROOT, "tests", "coassign_plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "coa_plan", [])


def _line(out, name):
    m = re.search(rf"^{name} cases (\d+) mismatches (\d+)$", out, re.M)
    assert m, (name, out)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("lb", WIDTHS)
@pytest.mark.parametrize("name,at_least", [("planes", 10**5), ("together", 97 * 400),
                                           ("onebit", 97 * 200)])
def test_planes_and_counts_equal_per_member_loops(check_output, name, lb, at_least):
    n, bad = _line(check_output, f"{name}{lb}")
    assert bad == 0
    assert n >= at_least


def test_plan_covers_entries_and_member_words_once_within_lds(check_output):
    n, bad = _line(check_output, "plan")
    assert bad == 0 and n >= 5 * 5000  # every n up to 5000 at every width, forced plans among them


def test_same_program_under_sanitizers(tmp_path_factory):
    """A stand-alone program: the sanitizer runtimes are linked into it."""
    out = _build_and_run(tmp_path_factory, "coa_plan_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for lb in WIDTHS:
        for name in ("planes", "together", "onebit"):
            assert _line(out, f"{name}{lb}")[1] == 0
    assert _line(out, "plan")[1] == 0


def test_build_info_hashes_the_coassign_sources():
    m = re.search(r" coa=([0-9a-f]{16})$", _lib.build_info())
    assert m, _lib.build_info()
    csrc = os.path.join(ROOT, "flipcomplexityempirical_amd", "csrc")
    blob = b"".join(open(os.path.join(csrc, f), "rb").read()
                    for f in ("fw_coassign.hip", "fw_coassign_plan.h"))
    assert m.group(1) == hashlib.sha256(blob).hexdigest()[:16], "library older than its sources"


def test_null_handles_are_refused_before_the_device():
    L = _lib.load()
    nodes = np.arange(3, dtype=np.int32)
    buf = np.zeros(9, np.uint64)
    info = np.zeros(7, np.int64)
    assert L.fw_chains_enable_coassign(None, _lib.ptr(nodes), 3) == _lib.FW_EINVAL
    assert L.fw_chains_enable_coassign(None, None, 0) == _lib.FW_EINVAL
    assert L.fw_chains_coassign_async(None) == _lib.FW_EINVAL
    assert L.fw_chains_read_coassign(None, _lib.COASSIGN_TOGETHER, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_write_coassign(None, _lib.COASSIGN_CNT, _lib.ptr(buf), buf.nbytes) == \
        _lib.FW_EINVAL
    assert L.fw_chains_coassign_reset(None) == _lib.FW_EINVAL
    assert L.fw_chains_coassign_info(None, _lib.ptr(info)) == _lib.FW_EINVAL
    assert L.fw_last_error().decode()


# ---- coassign.py against brute force on small random ensembles
def _ensemble(seed, chains=23, n=11, k=3, groups=1):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k, size=(chains * groups, n))
    rungs = np.tile(np.arange(groups), chains) if groups > 1 else None
    ref = coassign_ref.coassign(labels, k, None, rungs, groups)
    return labels, rungs, ref


@pytest.mark.parametrize("groups", [1, 3])
def test_scores_match_brute_force(groups):
    labels, rungs, ref = _ensemble(5 + groups, groups=groups)
    t, cnt = ref["together"], ref["cnt"]
    n = labels.shape[1]
    freq = coassign.frequency(t, cnt)
    assert freq.shape == t.shape
    for g in range(groups):
        members = labels if rungs is None else labels[rungs == g]
        for i in range(n):
            for j in range(n):
                want = np.mean(members[:, i] == members[:, j])
                assert freq[g, i, j] == pytest.approx(want, abs=1e-15)
    assert np.array_equal(coassign.separation(t, cnt), 1.0 - freq)
    sep = coassign.separation(t, cnt)
    # a pseudo-metric: the triangle inequality holds exactly on counts
    assert (sep[:, :, None, :] <= sep[:, :, :, None] + sep[:, None, :, :] + 1e-12).all()
    assert np.allclose(coassign.expected_mates(t, cnt), freq.sum(axis=2), rtol=0, atol=1e-12)
    h = coassign.pair_entropy(t, cnt)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = -(freq * np.log2(freq) + (1 - freq) * np.log2(1 - freq))
    want = np.where((freq > 0) & (freq < 1), want, 0.0)
    assert np.allclose(h, want, rtol=0, atol=1e-12) and (np.diagonal(h, axis1=1, axis2=2) == 0).all()
    pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)])
    cut = coassign.edge_cut_from_coassign(t, cnt, pairs)
    for g in range(groups):
        members = labels if rungs is None else labels[rungs == g]
        assert np.array_equal(cut[g], (members[:, pairs[:, 0]] != members[:, pairs[:, 1]])
                              .sum(axis=0).astype(np.uint64))
    # one group given as [m, m] and a scalar count
    assert np.array_equal(coassign.frequency(t[0], cnt[0]), freq[0])
    assert np.array_equal(coassign.edge_cut_from_coassign(t[0], cnt[0], pairs), cut[0])


@pytest.mark.parametrize("threshold", [0.3, 0.45, 0.6, 1.0])
def test_cores_are_networkx_components(threshold):
    import networkx as nx
    labels, _, ref = _ensemble(11, chains=17, n=14, k=2)
    # tie some nodes' fates so that high thresholds keep cores of more than one node
    labels[:, 1] = labels[:, 0]
    labels[:, 5] = labels[:, 4]
    labels[:10, 6] = labels[:10, 4]
    ref = coassign_ref.coassign(labels, 2)
    t, cnt = ref["together"], ref["cnt"]
    n = labels.shape[1]
    freq = coassign.frequency(t, cnt)[0]
    path = np.array([(i, i + 1) for i in range(n - 1)] + [(0, 7), (4, 6)])
    for edges in (None, path):
        got = coassign.cores(t, cnt, threshold, edges)[0]
        G = nx.Graph()
        G.add_nodes_from(range(n))
        cand = [(i, j) for i in range(n) for j in range(i + 1, n)] if edges is None else edges
        G.add_edges_from((int(i), int(j)) for i, j in cand if freq[i, j] >= threshold)
        comps = sorted(nx.connected_components(G), key=min)
        want = np.empty(n, np.int64)
        for label, comp in enumerate(comps):
            want[list(comp)] = label
        assert np.array_equal(got, want)
    assert np.array_equal(coassign.cores(t[0], cnt[0], threshold), coassign.cores(t, cnt, threshold)[0])
    if threshold == 1.0:
        assert got[0] == got[1] and got[4] == got[5]


def test_scores_refuse_malformed_input():
    with pytest.raises(ValueError):
        coassign.frequency(np.zeros((2, 3, 4)), np.ones(2))
    with pytest.raises(ValueError):
        coassign.frequency(np.zeros((2, 3, 3)), np.ones(3))
    with pytest.raises(ValueError):
        coassign.frequency(np.zeros((1, 3, 3)), np.zeros(1))
