"""The lean grid kernel's wave iteration against the CPU oracle, bit for bit.

Covers what the iteration's shortcuts rely on: the level-1 group-sum words read right after a
commit and carried into the next iteration (and across work units), the level-2 masks of
grids whose width is a multiple of 4 (a compile-time flag the plan sets) next to the general
ones, and the 32-bit sums of cut and |B| folded into the 64-bit totals.

The plan's fill model gives launches this small four rows per chain (the speculative
kernel, which has no width flag and ignores FLIPWALK_W2), so the R = 1 tests force
FLIPWALK_SPEC=1 and run under both register budgets of the lean kernel (FLIPWALK_W2=0: 3
waves per SIMD, the C3 kernel; FLIPWALK_W2=1: W2).  Every test reads the plan back from the
library's FLIPWALK_VERBOSE line and fails when another kernel than the intended one ran.
Final plans, populations, all stats fields (sum_invb bitwise) and both histograms must equal
oracle/flipchain_oracle.c.
"""
import pytest

from cases import MU, Case
from flipcomplexityempirical_amd.graph import band_seed, grid_graph
from test_gpu_parity import CASES, _run_vs_oracle

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in CASES}
# widths 5 and 7: the narrowest widths of the four-chains-per-wave kernel that are no
# multiple of 4 (every lane's four nodes wrap into the next grid row somewhere)
BY_NAME["grid12x5_k2"] = Case("grid12x5_k2", grid_graph(12, 5), band_seed(12, 5, 2), 2, 1, 0.20, 0.8)
BY_NAME["grid9x7_k3"] = Case("grid9x7_k3", grid_graph(9, 7), band_seed(9, 7, 3), 3, 1, 0.30, MU)

W4_GRIDS = ["grid12_k4_pairs", "grid20_k4_mu", "grid40x4_k2", "grid3x40_k2_bi"]  # W % 4 == 0
WX_GRIDS = ["grid10_k2_bi", "grid30x18_k2_bi", "grid12x5_k2", "grid9x7_k3"]      # W % 4 != 0


def _env(monkeypatch, rows, w2, **env):
    monkeypatch.delenv("FLIPWALK_NO_GRID16", raising=False)
    for k in ("FLIPWALK_SLICES", "FLIPWALK_GRID_CAP", "FLIPWALK_FOLD_AT", "FLIPWALK_GRID16_NW"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FLIPWALK_SPEC", rows)
    monkeypatch.setenv("FLIPWALK_W2", w2)
    monkeypatch.setenv("FLIPWALK_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(case, n_chains, steps_list, capfd, rows, w2):
    """_run_vs_oracle, then the plan the library printed: rows per chain, register budget
    and width flag must be the intended ones (2-bit labels: every case here has k <= 4)."""
    capfd.readouterr()
    st = _run_vs_oracle(case, n_chains, steps_list)
    plans = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("flipwalk: grid kernel")]
    assert plans, "no plan line: the grid kernel did not run"
    w4 = case.graph.grid_w % 4 == 0
    for ln in plans:
        assert f"2-bit labels, {rows} row(s) per chain" in ln, ln
        assert ("(W2 register budget)" in ln) == (rows == "1" and w2 == "1"), ln
        assert ("(W4 masks)" in ln) == (rows == "1" and w4), ln
    return st


@pytest.mark.parametrize("w2", ["0", "1"])
@pytest.mark.parametrize("name", W4_GRIDS + WX_GRIDS)
def test_width_flag_and_general_masks(gpu_lib, name, w2, monkeypatch, capfd):
    """Grids of widths 4, 12, 20 and 40 (the flag; W = 4 and a 3-row grid among them) and of
    widths 5, 7, 10 and 18 (the general masks): two launches, so the second one starts from
    the group sums carried in the record."""
    _env(monkeypatch, "1", w2)
    case = BY_NAME[name]
    assert (case.graph.grid_w % 4 == 0) == (name in W4_GRIDS)
    st = _run(case, 45, [400, 300], capfd, "1", w2)
    assert (st["accepts"] > 0).all()


@pytest.mark.parametrize("w2", ["0", "1"])
@pytest.mark.parametrize("name,slices", [("grid20_k4_mu", "3"), ("grid30x18_k2_bi", "7"),
                                         ("grid20_k4_mu", "7")])
def test_carried_level1_read_across_units(gpu_lib, name, slices, w2, monkeypatch, capfd):
    """One workgroup (FLIPWALK_GRID_CAP=1, at most 4 waves) runs 10 quads in 3 or 7 slices
    each: a wave's carried level-1 words must be re-read from every new unit's slot, never
    kept from the unit before."""
    _env(monkeypatch, "1", w2, FLIPWALK_GRID_CAP="1", FLIPWALK_SLICES=slices)
    _run(BY_NAME[name], 37, [600, 250], capfd, "1", w2)


@pytest.mark.parametrize("w2", ["0", "1"])
@pytest.mark.parametrize("fold_at", ["64", "4096"])
def test_sum_fold(gpu_lib, fold_at, w2, monkeypatch, capfd):
    """The 32-bit sums of cut and |B| fold into the 64-bit totals with the attempt counters.
    FLIPWALK_FOLD_AT=64 folds on the counters' trigger every few Philox refills; at 4096 the
    counters (sum_deg: about 5 per yield here) reach the threshold once in the run, while the
    sums (cut: about 65 per yield) pass it every ~60 yields, so nearly every fold is the sums'
    own trigger.  The totals must not change."""
    _env(monkeypatch, "1", w2, FLIPWALK_FOLD_AT=fold_at)
    st = _run(BY_NAME["grid20_k4_mu"], 13, [500, 700], capfd, "1", w2)
    at = int(fold_at)
    if at == 64:
        assert (st["sum_deg"] > 20 * at).all()  # many folds on the counters' trigger
    else:  # at most one fold on the counters' trigger, ten or more on the sums'
        assert (st["sum_deg"] < 2 * at).all() and (st["sum_cut"] > 10 * at).all()


@pytest.mark.parametrize("env", [{}, {"FLIPWALK_FOLD_AT": "64"}, {"FLIPWALK_FOLD_AT": "4096"},
                                 {"FLIPWALK_GRID_CAP": "1", "FLIPWALK_SLICES": "3"}],
                         ids=["plain", "fold", "sumfold", "units"])
@pytest.mark.parametrize("rows", ["2", "4"])
def test_speculative_rows(gpu_lib, rows, env, monkeypatch, capfd):
    """R = 2 and 4 rows per chain: every row of a group reads the level-1 words behind the
    committing row's update, and the owner row's sums fold group-uniformly (on the counters'
    trigger and on the sums' own)."""
    _env(monkeypatch, rows, "0", **env)
    _run(BY_NAME["grid20_k4_mu"], 37, [400, 300], capfd, rows, "0")
