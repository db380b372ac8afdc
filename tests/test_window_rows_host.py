"""The row-parallel 7x7 contiguity window (csrc/fw_window_rows.h) on the host.

The header holds the window's arithmetic as plain functions on 32-bit words, so
tests/window_rows_check.cpp compiles the same text with the host compiler, runs the seven
row-lanes of a chain as an array and compares the verdict with the oracle's
orc_window_verdict: every mask inside the central 5x5 (all source subsets), all subsets of
fixed sparse shapes (rings, spiral arms, corridors to each border side), more than 10^6
random 48-bit masks at densities 0.3, 0.5 and 0.7, and masks with rows and columns cut off
as at grid edges and corners; then the row-mask extraction for 2-, 3- and 4-bit labels
against a per-cell loop at every bit offset, and the column mask for every width up to 12.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler(names):
    for n in names:
        if n and shutil.which(n):
            return n
    return None


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cc = _compiler([os.environ.get("CC"), "cc", "gcc", "clang"])
    cxx = _compiler([os.environ.get("CXX"), "c++", "g++", "clang++"])
    if cc is None or cxx is None:
        pytest.skip("no host C / C++ compiler")
    d = tmp_path_factory.mktemp("window_rows")
    obj, exe = str(d / "oracle.o"), str(d / "window_rows_check")
    subprocess.run([cc, "-O2", "-std=c11", "-ffp-contract=off", "-c",
                    os.path.join(ROOT, "oracle", "flipchain_oracle.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread",
                    os.path.join(ROOT, "tests", "window_rows_check.cpp"), obj, "-lm", "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _line(out, name):
    m = re.search(rf"^{name} (?:masks|cases) (\d+) mismatches (\d+)(?: \(oracle: (\d+) undecided, "
                  rf"(\d+) open, (\d+) joined\))?$", out, re.M)
    assert m, (name, out)
    return [int(x) for x in m.groups() if x is not None]


@pytest.mark.parametrize("name,at_least", [("central5x5", 15 * 2**20), ("families", 10**6),
                                           ("random", 10**6), ("clipped", 10**6)])
def test_verdict_equals_oracle(check_output, name, at_least):
    n, bad, undecided, opened, joined = _line(check_output, name)
    assert bad == 0
    assert n >= at_least
    # the set exercises what it is meant to (the central 5x5 never reaches the border, so
    # nothing in it stays undecided)
    assert opened > 0 and joined > 0 and (undecided > 0 or name == "central5x5")


@pytest.mark.parametrize("name", ["row_mask2", "row_mask3", "row_mask4", "col_mask"])
def test_masks_equal_per_cell_loop(check_output, name):
    n, bad = _line(check_output, name)
    assert bad == 0 and n > 0
