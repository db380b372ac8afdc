"""The byte form of the grid kernel's level-2 weights (csrc/fw_weights_bytes.h) on the host.

The header holds the arithmetic as plain functions on 32-bit words, so
tests/weights_bytes_check.cpp compiles the same text with the host compiler, runs the 16
row-lanes of a chain as an array and compares every node's weight and cut degree with the
per-node rule of weights4<2, MODE>: every grid with W in {4, 8, ..., 40} and H in 1..40, every
group (and the one past the last, which the derive loop may visit), every lane, random labels
and labels biased to equal neighbours with k = 2, 3 and 4, for the pairs proposal (with and
without cut degrees) and the cut-edge proposal.  The chain's slot is laid out as the plan lays
it out with random bytes outside the labels, and every byte offset read must lie in
[-1, slot bytes).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++") if n and shutil.which(n)),
               None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("weights_bytes") / "weights_bytes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "weights_bytes_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("name", ["pairs", "pairs_cd", "cutedge"])
def test_weights_equal_per_node_rule(check_output, name):
    m = re.search(rf"^{name} cases (\d+) mismatches (\d+) out_of_slot (\d+) \(edge reads: (\d+) at -1, "
                  rf"(\d+) past the labels\)$", check_output, re.M)
    assert m, check_output
    cases, bad, oob, lo_edge, hi_edge = (int(x) for x in m.groups())
    assert bad == 0 and oob == 0
    # 10 widths x 40 heights x k = 2, 3, 4 x random / biased, every node of every group
    assert cases >= 10 * 40 * 3 * 2 * 64
    # the guard byte in front of the slot and bytes past the labels were read (and masked)
    assert lo_edge > 0 and hi_edge > 0


def test_perm_host_form(check_output):
    m = re.search(r"^perm cases (\d+) mismatches (\d+)$", check_output, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, check_output
