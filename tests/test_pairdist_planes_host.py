"""The pairwise plan distance's bit-plane arithmetic and blocking plan
(csrc/fw_pairdist_planes.h, csrc/fw_pairdist_plan.h) on the host.

The headers hold the arithmetic as plain functions on integers, so
tests/pairdist_planes_check.cpp compiles the same text with the host compiler and compares, for
each of the five label widths and every tail length 1..32, the XOR / OR / popcount count over
the planes with a per-field loop (random words, runs of few labels, pairs that differ only in
the fields that straddle a dword or in one bit of them), the planes themselves with the fields'
bits, and checks that the plan's chunks cover every group exactly once inside the LDS budget.
The program is built plainly and once more under the host compiler's address and
undefined-behaviour sanitizers; it is a stand-alone program, so their runtimes are linked into it.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 3, 4, 5, 8)


def _build_and_run(tmp_path_factory, name, extra):
    cxx = next((n for n in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp(name) / "pairdist_planes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *extra,
                    os.path.join(ROOT, "tests", "pairdist_planes_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "pwd_planes", [])


def _line(out, name):
    m = re.search(rf"^{name} cases (\d+) mismatches (\d+)$", out, re.M)
    assert m, (name, out)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("lb", WIDTHS)
@pytest.mark.parametrize("name,at_least", [("count", 3 * 10**5), ("runs", 10**5),
                                           ("straddle", 10**5), ("planes", 10**4)])
def test_plane_count_equals_per_field_loop(check_output, name, lb, at_least):
    n, bad = _line(check_output, f"{name}{lb}")
    assert bad == 0
    assert n >= at_least


def test_plan_covers_every_group_once_within_lds(check_output):
    n, bad = _line(check_output, "plan")
    assert bad == 0 and n >= 5 * 5000  # every n up to 5000 at every width, plus forced plans


def test_same_program_under_sanitizers(tmp_path_factory):
    """A stand-alone program: the sanitizer runtimes are linked into it."""
    out = _build_and_run(tmp_path_factory, "pwd_planes_san",
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for lb in WIDTHS:
        for name in ("count", "runs", "straddle", "planes"):
            assert _line(out, f"{name}{lb}")[1] == 0
    assert _line(out, "plan")[1] == 0
