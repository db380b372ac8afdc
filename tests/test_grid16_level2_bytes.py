"""The grid kernel's level-2 weights from byte-aligned label reads, against the CPU oracle.

On grids whose width is a multiple of 4 the lean R = 1 kernels (both register budgets) take a
lane's four labels, the rows above and below and the group's edge byte as single LDS bytes and
the left / right neighbours from the adjacent lanes (csrc/fw_weights_bytes.h), both in the
level-2 select of every attempt and in the derive loop of a handle's first launch.  Shapes
(W x H):

    4 x 16   a lane is a whole grid row: left and right neighbours always masked
    8 x 8    exactly one group
    12 x 12  group edges fall mid-row; a 16-node tail, lanes 4-15 past n; the derive loop
             visits the group past the last one
    20 x 20  several groups; up and down bytes cross group boundaries
    40 x 5   few rows: the first and last rows dominate

each with k = 2 (bi proposal), 3 (cut-edge proposal) and 4 (pairs proposal).  The plan's fill
model gives launches this small the speculative kernel, so every test forces FLIPWALK_SPEC=1,
runs under FLIPWALK_W2 = 0 and 1, reads the plan back from the FLIPWALK_VERBOSE line and fails
when another kernel than the intended one ran.  Final plans, populations, all stats fields
(sum_invb bitwise) and both histograms must equal oracle/flipchain_oracle.c.
"""
import numpy as np
import pytest

from cases import MU, Case
from flipcomplexityempirical_amd.graph import band_seed, grid_graph, stripe_seed
from test_gpu_parity import _run_vs_oracle

pytestmark = pytest.mark.gpu

SHAPES = [(4, 16), (8, 8), (12, 12), (20, 20), (40, 5)]  # W x H
MODE_OF_K = {2: 0, 3: 2, 4: 1}  # bi, cut-edge, pairs
BASE_OF_K = {2: 0.8, 3: MU, 4: 0.5}


def _col_seed(h, w, k):
    """Columns split into k vertical bands (40 x 5 has too few rows for k bands of rows)."""
    return np.repeat(((np.arange(w) * k) // w)[None, :], h, axis=0).astype(np.int16).reshape(-1)


def _case(w, h, k):
    seed = _col_seed(h, w, k) if h < 8 else band_seed(h, w, k)
    return Case(f"grid{w}x{h}_k{k}", grid_graph(h, w), seed, k, MODE_OF_K[k], 0.30, BASE_OF_K[k])


def _env(monkeypatch, w2, **env):
    for key in ("FLIPWALK_NO_GRID16", "FLIPWALK_SLICES", "FLIPWALK_GRID_CAP", "FLIPWALK_FOLD_AT",
                "FLIPWALK_GRID16_NW", "FLIPWALK_NO_BITBOARD", "FLIPWALK_NO_ROWBB"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("FLIPWALK_SPEC", "1")
    monkeypatch.setenv("FLIPWALK_W2", w2)
    monkeypatch.setenv("FLIPWALK_VERBOSE", "1")
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def _run(case, n_chains, steps_list, capfd, w2, w4=True):
    capfd.readouterr()
    st = _run_vs_oracle(case, n_chains, steps_list)
    plans = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("flipwalk: grid kernel")]
    assert plans, "no plan line: the grid kernel did not run"
    for ln in plans:
        assert "small-grid plan" in ln and "2-bit labels, 1 row(s) per chain" in ln, ln
        assert ("(W2 register budget)" in ln) == (w2 == "1"), ln
        assert ("(W4 masks)" in ln) == w4, ln
    assert (st["accepts"] > 0).all()
    return st


@pytest.mark.parametrize("w2", ["0", "1"])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_level2_bytes_bit_exact(gpu_lib, shape, k, w2, monkeypatch, capfd):
    """Two launches: the first derives the group sums with the byte form (NEED_CD), the second
    starts from the sums carried in the record; every attempt's level 2 is the byte form."""
    _env(monkeypatch, w2)
    _run(_case(*shape, k), 24, [1200, 800], capfd, w2)


@pytest.mark.parametrize("w2", ["0", "1"])
def test_uncached_derive_only(gpu_lib, w2, monkeypatch, capfd):
    """A fresh handle's first and only launch on 12 x 12 (three groups: the derive loop's
    second pair holds the group past the last one): cut, |B| and the proposal count of the
    initial plan come from the byte form alone."""
    _env(monkeypatch, w2)
    st = _run(_case(12, 12, 4), 24, [2000], capfd, w2)
    assert (st["yields"] == 2001).all()


@pytest.mark.parametrize("w2", ["0", "1"])
def test_sliced_units(gpu_lib, w2, monkeypatch, capfd):
    """One workgroup runs every quad in three slices: only a quad's first slice derives, the
    later ones load the sums the slice before wrote back."""
    _env(monkeypatch, w2, FLIPWALK_GRID_CAP="1", FLIPWALK_SLICES="3")
    _run(_case(20, 20, 4), 37, [1500, 900], capfd, w2)


@pytest.mark.parametrize("w2", ["0", "1"])
def test_other_widths_keep_the_window_form(gpu_lib, w2, monkeypatch, capfd):
    """10 x 10: the width is no multiple of 4, so the plan must not set the flag and the
    dword-window form runs and still matches."""
    _env(monkeypatch, w2)
    case = Case("grid10_k2_bi", grid_graph(10, 10), stripe_seed(10, 10), 2, 0, 0.10, MU)
    _run(case, 24, [1200, 800], capfd, w2, w4=False)
