"""The plan-overlap kernel's field arithmetic (csrc/fw_overlap_bits.h) on the host.

The header holds the arithmetic as plain functions on 32-bit words, so
tests/overlap_bits_check.cpp compiles the same text with the host compiler and compares, for
each of the five label widths, the "field equals value" mask, the pair mask, the
differing-fields mask and the field extraction with a per-field loop over more than 10^6 word
groups (random words, runs of few labels, and pairs that differ only in the fields that
straddle a dword), and the tail mask at every length 1..32.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 3, 4, 5, 8)


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("overlap_bits") / "overlap_bits_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "overlap_bits_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _line(out, name):
    m = re.search(rf"^{name} cases (\d+) mismatches (\d+)$", out, re.M)
    assert m, (name, out)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("lb", WIDTHS)
@pytest.mark.parametrize("name,at_least", [("eq", 10**6), ("pair", 10**6), ("diff", 10**6),
                                           ("field", 10**6), ("straddle", 10**5)])
def test_masks_equal_per_field_loop(check_output, name, lb, at_least):
    n, bad = _line(check_output, f"{name}{lb}")
    assert bad == 0
    assert n >= at_least


def test_tail_mask_at_every_length(check_output):
    assert _line(check_output, "tail") == (32, 0)
