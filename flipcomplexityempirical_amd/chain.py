"""Batched flip-walk chains on MI355X (host side of the drop-in boundary).

``Chains`` is the batched form of the reference's

    MarkovChain(slow_reversible_propose_bi, Validator([single_flip_contiguous, popbound]),
                accept=cut_accept, initial_state=grid_partition, total_steps=100000)

(grid_chain_sec11.py:340-342): thousands of independent chains, one per Philox
stream, advanced by the HIP kernel through the C-ABI.  Host-side numerics that
the kernels take as inputs are computed here exactly as the reference computes
them in Python:

* ``population_bounds`` — ``within_percent_of_ideal_population`` (grid_chain_sec11.py:319):
  ideal = sum(pops)/k, (1-p)*ideal <= pop <= (1+p)*ideal with Python floats, turned
  into the equivalent integer interval [ceil(lo), floor(hi)].
* ``metropolis_table`` — ``cut_accept`` (grid_chain_sec11.py:171-179): bound =
  base ** (len(parent cut) - len(cut)) = base ** (-Δcut) with Python's float pow.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import STATS_DTYPE, check, ptr
from .graph import Graph

DEFAULT_MAX_RETRIES = 1 << 20

PROPOSALS = {"bi": _lib.PROPOSE_BI, "pairs": _lib.PROPOSE_PAIRS, "cutedge": _lib.PROPOSE_CUTEDGE}


def population_bounds(total_pop: int, k: int, percent: float):
    """Integer bounds equivalent to GerryChain's Bounds((1-p)*ideal, (1+p)*ideal)."""
    ideal = total_pop / k
    lo = (1 - percent) * ideal
    hi = (1 + percent) * ideal
    return int(math.ceil(lo)), int(math.floor(hi))


def metropolis_table(base: float, maxdeg: int) -> np.ndarray:
    """thr[d + maxdeg] = base ** (-d): cut_accept's bound for Δcut = d."""
    b = float(base)
    return np.array([b ** (-d) for d in range(-maxdeg, maxdeg + 1)], dtype=np.float64)


def annealing_table(base: float, beta: float, maxdeg: int) -> np.ndarray:
    """thr[d + maxdeg] = base ** (beta * (-d)): the power of annealing_cut_accept_backwards
    (grid_chain_sec11.py:101), base**(beta*(-len(cut)+len(parent cut))), for Δcut = d."""
    b = float(base)
    return np.array([b ** (beta * (-d)) for d in range(-maxdeg, maxdeg + 1)], dtype=np.float64)


def reference_beta(t: int):
    """The commented beta schedule of annealing_cut_accept_backwards
    (grid_chain_sec11.py:88-93) at step_num t: 0 before 100,000, a linear ramp to 3 at
    400,000, then 3 (Python int / float values as the reference writes them)."""
    if t < 100000:
        return 0
    if t < 400000:
        return (t - 100000) / 100000
    return 3


def schedule_rows(base: float, beta_of_t, t_start: int, t_stop: int,
                  maxdeg: int) -> tuple[np.ndarray, int]:
    """Rows for ``Chains.set_schedule``: row i = annealing_table(base, beta_of_t(t_start+i))
    for step_num t_start..t_stop; returns (rows, t0 = t_start).  Exact when beta_of_t is
    constant for t <= t_start and for t >= t_stop (the kernel clamps to the end rows).
    Each power is CPython's float pow, as in the reference."""
    rows = np.empty((t_stop - t_start + 1, 2 * maxdeg + 1), np.float64)
    cache = {}
    for i in range(rows.shape[0]):
        beta = beta_of_t(t_start + i)
        key = (type(beta), beta)
        if key not in cache:
            cache[key] = annealing_table(base, beta, maxdeg)
        rows[i] = cache[key]
    return rows, t_start


ACCEPT_RULES = {"cut": _lib.ACCEPT_CUT, "bratio": _lib.ACCEPT_BRATIO,
                "boundary": _lib.ACCEPT_BOUNDARY}

MAX_RUNGS = 64  # one wave per replica set, one lane per rung (fw_chains_exchange_async)

SERIES_KINDS = {"cut": _lib.SERIES_CUT, "bnodes": _lib.SERIES_BNODES, "rung": _lib.SERIES_RUNG}

OVERLAP_KINDS = {"reference": _lib.OVERLAP_REFERENCE, "partner": _lib.OVERLAP_PARTNER}


def ladder_layout(n_chains: int, n_rungs: int):
    """The default placement of ``Chains.set_ladder``: consecutive chains form a replica
    set, (set_of_chain, rung_of_chain) = (c // n_rungs, c % n_rungs)."""
    c = np.arange(int(n_chains), dtype=np.int32)
    return c // np.int32(n_rungs), c % np.int32(n_rungs)


def check_ladder_layout(n_chains: int, n_rungs: int, set_of_chain, rung_of_chain):
    """fw_chains_set_ladder's host validation (ValueError instead of FW_EINVAL): 2 <= n_rungs
    <= 64 divides n_chains, set ids lie in [0, n_chains / n_rungs) and every (set, rung)
    holds exactly one chain.  Returns the two arrays as contiguous int32."""
    n_chains, n_rungs = int(n_chains), int(n_rungs)
    if not 2 <= n_rungs <= MAX_RUNGS:
        raise ValueError(f"n_rungs = {n_rungs} outside [2, {MAX_RUNGS}]")
    if n_chains % n_rungs:
        raise ValueError(f"{n_chains} chains are not a multiple of {n_rungs} rungs")
    s = np.ascontiguousarray(set_of_chain, np.int32)
    r = np.ascontiguousarray(rung_of_chain, np.int32)
    if s.shape != (n_chains,) or r.shape != (n_chains,):
        raise ValueError(f"set_of_chain and rung_of_chain must be [{n_chains}]")
    n_sets = n_chains // n_rungs
    if (s < 0).any() or (s >= n_sets).any() or (r < 0).any() or (r >= n_rungs).any():
        raise ValueError(f"(set, rung) outside [0, {n_sets}) x [0, {n_rungs})")
    count = np.bincount(s.astype(np.int64) * n_rungs + r, minlength=n_chains)
    if (count != 1).any():
        slot = int(np.flatnonzero(count != 1)[0])
        raise ValueError(f"rung {slot % n_rungs} of set {slot // n_rungs} holds "
                         f"{int(count[slot])} chains: every (set, rung) needs exactly one")
    return s, r


def check_geometry_arrays(n: int, n_edges: int, edge_weights=None, area=None, exterior=None):
    """fw_chains_set_geometry's host validation (ValueError instead of FW_EINVAL), before the
    library is called: each array is None or integers of shape [n_edges] (``edge_weights``) or
    [n] (``area``, ``exterior``), every value >= 0 and every total below 2^31.  Returns the
    three as contiguous int64 arrays (or None)."""
    out = []
    for name, a, length in (("edge_weights", edge_weights, n_edges), ("area", area, n),
                            ("exterior", exterior, n)):
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integers, got {a.dtype} "
                             "(compactness.quantise turns lengths and areas into them)")
        if a.shape != (int(length),):
            raise ValueError(f"{name} must be [{int(length)}], got {a.shape}")
        if a.size and int(a.min()) < 0:
            raise ValueError(f"{name} must be >= 0")
        if a.size and (int(a.max()) >= 2 ** 31 or int(a.astype(np.uint64).sum()) >= 2 ** 31):
            raise ValueError(f"the total of {name} must stay below 2^31")
        out.append(np.ascontiguousarray(a, np.int64))
    return tuple(out)


def expected_wait_sum(stats, n_nodes: int, k: int) -> np.ndarray:
    """Σ_t E[geom_wait_t] = (N^k - 1) * Σ 1/|B_t| - T (geom_wait, grid_chain_sec11.py:147-148)."""
    M = float(n_nodes ** k - 1)
    return M * stats["sum_invb"] - stats["yields"].astype(np.float64)


def wait_prob_table(n_nodes: int, k: int) -> np.ndarray:
    """p_b = len(b_nodes) / (N**k - 1) for every boundary size b = 0..N, divided as
    geom_wait divides (grid_chain_sec11.py:148: Python int / int, correctly rounded)."""
    M = int(n_nodes) ** int(k) - 1
    return np.array([b / M for b in range(int(n_nodes) + 1)], np.float64)


def write_wait_txt(path: str, wait_sum: float) -> None:
    """The reference's only text output (grid_chain_sec11.py:410-411):
    ``wfile.write(str(sum(waits)))``.  ``wait_sum`` is either the sampled sum
    (``Chains.sampled_waits``, the reference's own kind of value: a sum of integer draws)
    or the Rao-Blackwellised expectation (expected_wait_sum), written as the nearest
    integer."""
    with open(path, "w") as f:
        f.write(str(int(round(float(wait_sum)))))


class DeviceGraph:
    """A CSR graph uploaded to one HIP device (fw_graph)."""

    def __init__(self, graph: Graph, device: int = 0):
        L = _lib.require_device()
        self.graph = graph
        self.device = device
        h = _lib.ctypes.c_void_p()
        rowptr = np.ascontiguousarray(graph.rowptr, np.int32)
        col = np.ascontiguousarray(graph.col, np.int32)
        pop = None if graph.pop is None else np.ascontiguousarray(graph.pop, np.int64)
        check(L.fw_graph_create(ptr(rowptr), ptr(col), ptr(pop), graph.n, len(col), device,
                                _lib.ctypes.byref(h)))
        self._h = h
        # handles of the chains created on this graph and not yet closed: fw_chains keeps a
        # pointer to its fw_graph, so they must be destroyed before it (close)
        self._live = {}
        info = np.zeros(5, np.int64)
        check(L.fw_graph_info(self._h, ptr(info)))
        self.n, self.n_edges, self.maxdeg, self.grid_w, self.grid_h = (int(x) for x in info)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            # the garbage collector may finalise a graph before its chains: destroy them
            # first (their Chains objects see the cleared handle and do nothing more)
            for h in list(self._live.values()):
                if h.value:
                    _lib.load().fw_chains_destroy(h)
                    h.value = None
            self._live.clear()
            _lib.load().fw_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Chains:
    """n_chains independent flip walks resident on one device (fw_chains)."""

    def __init__(self, dgraph: DeviceGraph, n_chains: int, k: int, init_labels,
                 proposal: str | int = "pairs", pop_bounds=None, percent: float = 0.05,
                 base: float | Sequence[float] = 1.0, seed: int = 0, chain_id0: int = 0,
                 thr: Optional[np.ndarray] = None):
        L = _lib.require_device()
        self.dgraph = dgraph
        g = dgraph.graph
        self.n_chains, self.k = int(n_chains), int(k)
        self.mode = PROPOSALS[proposal] if isinstance(proposal, str) else int(proposal)
        lab = np.ascontiguousarray(init_labels, np.int16)
        if lab.ndim == 2 and lab.shape[0] not in (1, n_chains):
            raise ValueError(f"init_labels has {lab.shape[0]} rows: need 1 or n_chains={n_chains}")
        if lab.ndim not in (1, 2) or lab.shape[-1] != g.n:
            raise ValueError(f"init_labels must be [{g.n}] or [rows, {g.n}], got {lab.shape}")
        per_chain = 1 if lab.ndim == 2 and lab.shape[0] == n_chains and n_chains > 1 else 0
        if lab.ndim == 2 and not per_chain:
            lab = np.ascontiguousarray(lab[0])
        if pop_bounds is None:
            pop_bounds = population_bounds(g.total_pop, k, percent)
        self.pop_lo, self.pop_hi = int(pop_bounds[0]), int(pop_bounds[1])
        D = dgraph.maxdeg
        if thr is not None:  # an explicit bound table [2*maxdeg+1] or [n_chains][2*maxdeg+1]
            thr = np.asarray(thr, np.float64)
            thr_per = 1 if thr.ndim == 2 else 0
        elif np.ndim(base) == 0:
            thr = metropolis_table(float(base), D)
            thr_per = 0
        else:
            bases = np.asarray(base, np.float64)
            if len(bases) != n_chains:
                raise ValueError("per-chain bases need one base per chain")
            thr = np.stack([metropolis_table(float(b), D) for b in bases])
            thr_per = 1
        self.thr = np.ascontiguousarray(thr)
        self.seed, self.chain_id0 = int(seed), int(chain_id0)
        # the configuration a checkpoint must carry besides the state (set_accept,
        # set_schedule change it after creation)
        self.accept_rule, self.node_flags = _lib.ACCEPT_CUT, None
        self._sched, self._sched_t0 = None, 0
        self.waits_on = False
        self.ladder_bases, self.set_of_chain, self.ladder_round = None, None, 0
        # enable_series: the capacity and, per sample, the ladder epoch of its rung row (a
        # mirror of the handle's stamps, which a checkpoint carries as a validity mask)
        self.series_capacity, self._series_epoch = 0, None
        # set_columns / set_elections: what a checkpoint carries of the tally besides the
        # histogram; _tally_base is the n_tallied a restored checkpoint started from
        self.columns, self.column_names, self.elections = None, None, None
        self._tally_base = 0
        # set_geometry: the three arrays a checkpoint carries (None: unit weights, unit areas,
        # no exterior); _geometry_base as _tally_base
        self.geometry_arrays = None
        self._geometry_base = 0
        # set_partners: the array a checkpoint carries (the reference is read back from the
        # handle); _overlap_base as _tally_base
        self.partners = None
        self._overlap_base = 0
        self._census_base = 0  # as _overlap_base, for the ensemble census
        self._pairdist_base = 0  # and for the pairwise plan distances
        # enable_coassignment: the caller's node order as positions in the sorted list the
        # handle holds (None: not enabled); _coassign_base as _census_base
        self._coassign_order = None
        self._coassign_base = 0
        # clone / resample: the round the next resample() takes by default, and the counts a
        # restored checkpoint started from (as _tally_base)
        self.resample_round = 0
        self._resample_base, self._clone_base = 0, 0
        h = _lib.ctypes.c_void_p()
        check(L.fw_chains_create(dgraph.handle, self.n_chains, self.k, ptr(lab), per_chain,
                                 self.mode, self.pop_lo, self.pop_hi, ptr(self.thr), thr_per,
                                 self.seed & (2**64 - 1), self.chain_id0, _lib.ctypes.byref(h)))
        self._h = h
        dgraph._live[id(h)] = h

    # ------------------------------------------------------------- stepping
    def run(self, steps: int, max_retries: int = DEFAULT_MAX_RETRIES) -> None:
        check(_lib.load().fw_chains_run(self._h, int(steps), int(max_retries)))

    def run_async(self, steps: int, max_retries: int = DEFAULT_MAX_RETRIES) -> None:
        check(_lib.load().fw_chains_run_async(self._h, int(steps), int(max_retries)))

    def sync(self) -> None:
        check(_lib.load().fw_chains_sync(self._h))

    def run_traced(self, steps: int, max_retries: int = DEFAULT_MAX_RETRIES) -> np.ndarray:
        tr = np.empty((self.n_chains, int(steps)), np.int32)
        check(_lib.load().fw_chains_run_traced(self._h, int(steps), int(max_retries), ptr(tr),
                                               tr.nbytes))
        return tr

    def last_kernel_ms(self) -> float:
        return float(_lib.load().fw_chains_last_kernel_ms(self._h))

    def launch_info(self) -> dict:
        """The launch plan (fw_chains_launch_info) and the residency it gives: waves per SIMD
        and chains per CU of the persistent grid (4 SIMDs per CU)."""
        info = np.zeros(8, np.int64)
        check(_lib.load().fw_chains_launch_info(self._h, ptr(info)))
        wgs, nw, cpw, lds, vgpr, scratch, cus, per_cu = (int(x) for x in info)
        resident = min(wgs, per_cu * cus)
        return {"workgroups": wgs, "waves_per_workgroup": nw, "chains_per_wave": cpw,
                "lds_bytes_per_workgroup": lds, "vgprs": vgpr, "scratch_bytes_per_lane": scratch,
                "cus": cus, "workgroups_per_cu": per_cu,
                "waves_per_simd_limit": per_cu * nw / 4.0,
                "waves_per_simd": resident * nw / (4.0 * cus),
                "chains_per_cu": resident * nw * cpw / cus}

    def reset_observables(self) -> None:
        check(_lib.load().fw_chains_reset_observables(self._h))

    # ------------------------------------------------------------- reading
    def _read(self, what, arr):
        check(_lib.load().fw_chains_read(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def labels(self) -> np.ndarray:
        return self._read(_lib.READ_LABELS, np.empty((self.n_chains, self.dgraph.n), np.int16))

    def stats(self) -> np.ndarray:
        return self._read(_lib.READ_STATS, np.empty(self.n_chains, STATS_DTYPE))

    def hist_cut(self) -> np.ndarray:
        return self._read(_lib.READ_HIST_CUT, np.empty(self.dgraph.n_edges + 1, np.uint64))

    def hist_b(self) -> np.ndarray:
        return self._read(_lib.READ_HIST_B, np.empty(self.dgraph.n + 1, np.uint64))

    def pops(self) -> np.ndarray:
        return self._read(_lib.READ_POPS, np.empty((self.n_chains, self.k), np.int64))

    def set_accept(self, rule: str | int, node_flags=None) -> None:
        """Accept rule: "cut" (cut_accept), "bratio" (annealing_cut_accept_backwards' |B'|/|B|
        factor on the tabulated power) or "boundary" (uniform_accept + boundary_condition
        over ``node_flags``, the boundary_node attribute); see include/flipwalk.h."""
        r = ACCEPT_RULES[rule] if isinstance(rule, str) else int(rule)
        fl = None if node_flags is None else np.ascontiguousarray(node_flags, np.uint8)
        check(_lib.load().fw_chains_set_accept(self._h, r, ptr(fl)))
        self.accept_rule, self.node_flags = r, fl

    def set_schedule(self, rows=None, t0: int = 0) -> None:
        """Step-dependent bounds shared by every chain (fw_chains_set_schedule): a proposal
        with step_num t (accepted flips + 1, grid_chain_sec11.py:282-289) uses row
        clamp(t - t0, 0, len(rows) - 1) in place of the thr table.  ``rows=None`` removes
        it.  See ``schedule_rows``."""
        if rows is None:
            check(_lib.load().fw_chains_set_schedule(self._h, None, 0, 0))
            self._sched, self._sched_t0 = None, 0
            return
        r = np.ascontiguousarray(rows, np.float64)
        if r.ndim != 2 or r.shape[1] != self.thr.shape[-1]:
            raise ValueError(f"schedule rows must be [n][{self.thr.shape[-1]}]")
        check(_lib.load().fw_chains_set_schedule(self._h, ptr(r), r.shape[0], int(t0)))
        self._sched, self._sched_t0 = r, int(t0)

    # ------------------------------------------------------------- replica exchange
    def set_ladder(self, bases, set_of_chain=None, rung_of_chain=None) -> None:
        """Join the chains into replica sets over a ladder of Metropolis bases
        (fw_chains_set_ladder): rung r runs cut_accept with ``bases[r]``, and ``exchange``
        lets neighbouring rungs of a set trade places.  The default placement is
        ``ladder_layout``.  Needs the "cut" accept rule and no schedule.  Zeroes the rung
        stats and restarts ``ladder_round``."""
        bases = np.array(bases, np.float64).ravel()
        if (set_of_chain is None) != (rung_of_chain is None):
            raise ValueError("give both set_of_chain and rung_of_chain, or neither")
        if set_of_chain is None:
            set_of_chain, rung_of_chain = ladder_layout(self.n_chains, max(len(bases), 1))
        s, r = check_ladder_layout(self.n_chains, len(bases), set_of_chain, rung_of_chain)
        rows = np.ascontiguousarray(
            np.stack([metropolis_table(float(b), self.dgraph.maxdeg) for b in bases]))
        logb = np.array([math.log(float(b)) for b in bases], np.float64)
        check(_lib.load().fw_chains_set_ladder(self._h, ptr(rows), ptr(logb), len(bases),
                                               ptr(s), ptr(r)))
        self.ladder_bases, self.set_of_chain, self.ladder_round = bases, s, 0
        self._coassign_base = 0  # the handle re-sized and zeroed the co-assignment by rung

    @property
    def n_rungs(self) -> int:
        return 0 if self.ladder_bases is None else len(self.ladder_bases)

    def exchange(self, round: int) -> None:
        """One exchange step on the handle's stream (fw_chains_exchange_async): pairs
        (r, r+1) with r = round (mod 2) swap with probability min(1, (b_r / b_{r+1}) **
        (cut_r - cut_{r+1})).  The draw is a function of (seed, round, set, r)."""
        check(_lib.load().fw_chains_exchange_async(self._h, int(round)))

    def rungs(self) -> np.ndarray:
        """int32 [n_chains]: the rung each chain sits on now."""
        return self._read(_lib.READ_RUNG, np.empty(self.n_chains, np.int32))

    def rung_stats(self) -> np.ndarray:
        """RUNG_STATS_DTYPE [n_sets, n_rungs]: yields, steps, accepts and the cut / boundary
        sums of whichever chains sat on the rung, as of the last exchange, and the swaps
        tried / done with the rung above."""
        return self._read(_lib.READ_RUNG_STATS,
                          np.empty((self.n_chains // self.n_rungs, self.n_rungs),
                                   _lib.RUNG_STATS_DTYPE))

    def run_tempered(self, steps_per_round: int, n_rounds: int, round0: Optional[int] = None,
                     max_retries: int = DEFAULT_MAX_RETRIES, record: bool = False,
                     tally: bool = False, geometry: bool = False,
                     overlap: bool | str = False, census: bool = False,
                     coassign: bool = False) -> None:
        """``n_rounds`` x (``steps_per_round`` steps, one exchange), enqueued back to back and
        waited for once.  Rounds are numbered from ``round0`` (default: where the last call
        stopped, ``ladder_round``), which fixes the parity and the draws of each exchange.
        With ``record`` every round is run, record, exchange: a series sample carries the rung
        its chain has just run on; with ``tally`` every round is run, tally, exchange, so a
        plan is counted under that rung too, and with ``geometry`` its districts are measured
        under it, and with ``overlap`` (True: against the reference, or "partner") its distance
        is binned under it, and with ``census`` it enters the ensemble maps of that rung, and
        with ``coassign`` the co-assignment matrix of that rung (run, tally, geometry, overlap,
        census, coassign, record, exchange)."""
        if self.ladder_bases is None:
            raise ValueError("run_tempered needs a ladder (set_ladder)")
        r0 = self.ladder_round if round0 is None else int(round0)
        L = _lib.load()
        for i in range(int(n_rounds)):
            check(L.fw_chains_run_async(self._h, int(steps_per_round), int(max_retries)))
            if tally:
                self.tally()
            if geometry:
                self.geometry()
            if overlap:
                self.overlap("reference" if overlap is True else overlap)
            if census:
                self.census()
            if coassign:
                self.coassign()
            if record:
                self.record()
            check(L.fw_chains_exchange_async(self._h, r0 + i))
        self.sync()
        self.ladder_round = r0 + int(n_rounds)

    # ------------------------------------------------------------- observable series
    def enable_series(self, capacity: int) -> None:
        """Keep up to ``capacity`` thinned samples of every chain's cut and boundary size
        (and rung, under a ladder) on the device (fw_chains_enable_series); once per handle."""
        check(_lib.load().fw_chains_enable_series(self._h, int(capacity)))
        self.series_capacity = int(capacity)
        self._series_epoch = np.zeros(int(capacity), np.int64)

    def series_info(self) -> dict:
        info = np.zeros(4, np.int64)
        check(_lib.load().fw_chains_series_info(self._h, ptr(info)))
        return {"capacity": int(info[0]), "n_samples": int(info[1]), "epoch": int(info[2]),
                "n_rungs": int(info[3])}

    @property
    def n_samples(self) -> int:
        return self.series_info()["n_samples"]

    def record(self) -> None:
        """One sample of every chain, enqueued on the handle's stream behind the runs already
        there (fw_chains_record_async); no wait."""
        check(_lib.load().fw_chains_record_async(self._h))
        info = self.series_info()
        self._series_epoch[info["n_samples"] - 1] = info["epoch"]

    def series_reset(self) -> None:
        check(_lib.load().fw_chains_series_reset(self._h))

    def _series_window(self, t0, n):
        t0 = int(t0)
        return t0, (self.n_samples - t0 if n is None else int(n))

    def series(self, what: str | int, by_rung: bool = False, t0: int = 0,
               n: Optional[int] = None) -> np.ndarray:
        """int32 [n, n_chains]: samples t0 .. t0 + n - 1 (default: to the last) of "cut",
        "bnodes" or "rung", one column per chain; with ``by_rung`` one column per
        (set, rung) slot, set * n_rungs + rung, holding the chain that sat there."""
        kind = SERIES_KINDS[what] if isinstance(what, str) else int(what)
        t0, n = self._series_window(t0, n)
        out = np.empty((max(n, 0), self.n_chains), np.int32)
        if n == 0:
            return out
        check(_lib.load().fw_chains_read_series(
            self._h, kind | (_lib.SERIES_BY_RUNG if by_rung else 0), t0, n, ptr(out), out.nbytes))
        return out

    def write_series(self, what: str | int, values, t0: int = 0) -> None:
        """Overwrite samples t0 .. of a series from int32 [n, n_chains] (checkpoints, tests);
        see fw_chains_write_series for what is validated."""
        kind = SERIES_KINDS[what] if isinstance(what, str) else int(what)
        a = np.ascontiguousarray(values, np.int32)
        if a.ndim != 2 or a.shape[1] != self.n_chains:
            raise ValueError(f"series values must be [n, {self.n_chains}]")
        before = self.n_samples if self.series_capacity else 0
        check(_lib.load().fw_chains_write_series(self._h, kind, int(t0), a.shape[0], ptr(a),
                                                 a.nbytes))
        lo, hi = int(t0), int(t0) + a.shape[0]
        if kind == _lib.SERIES_RUNG:
            self._series_epoch[lo:hi] = self.series_info()["epoch"]
        elif hi > before:
            self._series_epoch[before:hi] = 0

    def series_acf(self, what: str | int, max_lag: int, by_rung: bool = False, t0: int = 0,
                   n: Optional[int] = None, per_series: bool = False):
        """Pooled autocovariance sums of the window's series (fw_chains_series_acf): float64
        [n_groups, max_lag + 3] = {sum over series of c[0..max_lag], of the means, of their
        squares}; one group, or with ``by_rung`` one per rung.  ``per_series`` also returns
        the exact int64 sums [n_series, 3, max_lag + 1] = {P, A, B}.  ``diagnostics`` turns
        the pooled rows into autocorrelations, tau_int, ESS and R-hat."""
        kind = SERIES_KINDS[what] if isinstance(what, str) else int(what)
        t0, n = self._series_window(t0, n)
        groups = self.n_rungs if by_rung and self.n_rungs else 1
        pooled = np.empty((groups, int(max_lag) + 3), np.float64)
        ps = np.empty((self.n_chains, 3, int(max_lag) + 1), np.int64) if per_series else None
        check(_lib.load().fw_chains_series_acf(
            self._h, kind | (_lib.SERIES_BY_RUNG if by_rung else 0), t0, n, int(max_lag),
            ptr(ps), ptr(pooled)))
        return (pooled, ps) if per_series else pooled

    def run_sampled(self, steps_per_sample: int, n_samples: int,
                    max_retries: int = DEFAULT_MAX_RETRIES, tally: bool = False,
                    geometry: bool = False, overlap: bool | str = False,
                    census: bool = False, pairs=False, coassign: bool = False) -> None:
        """``n_samples`` x (``steps_per_sample`` steps, one recorded sample), enqueued back to
        back and waited for once.  With ``tally`` every sample's plans are tallied as well, with
        ``geometry`` their districts are measured, with ``overlap`` (True: against the
        reference, or "partner") they are compared, with ``census`` they enter the ensemble maps,
        with ``pairs`` (True: all chains, or a member list) their pairwise distances are measured,
        with ``coassign`` they enter the node co-assignment matrix (run, tally, geometry, overlap,
        census, coassign, pairs, record)."""
        L = _lib.load()
        for _ in range(int(n_samples)):
            check(L.fw_chains_run_async(self._h, int(steps_per_sample), int(max_retries)))
            if tally:
                self.tally()
            if geometry:
                self.geometry()
            if overlap:
                self.overlap("reference" if overlap is True else overlap)
            if census:
                self.census()
            if coassign:
                self.coassign()
            if pairs is not False and pairs is not None:
                self.pair_distances(None if pairs is True else pairs)
            self.record()
        self.sync()

    # ------------------------------------------------------------- district tallies
    def set_columns(self, cols) -> None:
        """Node columns to sum per district (fw_chains_set_columns): an integer array
        [n_cols, n] (or [n] for one column), or a dict name -> [n] whose insertion order
        gives the column indices and whose names are kept in ``column_names``.  1 to 8
        columns, values >= 0, every column's total below 2^31.  Replaces earlier columns,
        drops the elections and zeroes the seat histogram."""
        names = None
        if isinstance(cols, dict):
            names = [str(name) for name in cols]
            if not names:
                raise ValueError("no columns given")
            cols = [np.asarray(v) for v in cols.values()]
            if any(c.shape != (self.dgraph.n,) for c in cols):
                raise ValueError(f"every column must be [{self.dgraph.n}]")
            cols = np.stack(cols)
        a = np.asarray(cols)
        if a.dtype.kind not in "iub":
            raise ValueError(f"columns must be integers, got {a.dtype}")
        if a.dtype.kind == "u" and a.size and int(a.max()) >= 2 ** 63:
            raise ValueError("column value outside int64")
        a = np.ascontiguousarray(np.atleast_2d(a), np.int64)
        if a.ndim != 2 or a.shape[1] != self.dgraph.n:
            raise ValueError(f"columns must be [n_cols, {self.dgraph.n}], got {a.shape}")
        check(_lib.load().fw_chains_set_columns(self._h, ptr(a), a.shape[0]))
        self.columns, self.column_names = a, names
        self.elections = np.zeros((0, 2), np.int32)

    def _column_index(self, c) -> int:
        if isinstance(c, str):
            if not self.column_names or c not in self.column_names:
                raise ValueError(f"no column named {c!r}")
            return self.column_names.index(c)
        return int(c)

    def set_elections(self, pairs) -> None:
        """Elections between two columns each (fw_chains_set_elections): up to 4 pairs
        (a, b) of distinct column indices or names.  Zeroes the seat histogram."""
        ab = np.array([[self._column_index(a), self._column_index(b)] for a, b in pairs],
                      np.int32).reshape(-1, 2)
        ab = np.ascontiguousarray(ab)
        check(_lib.load().fw_chains_set_elections(self._h, ptr(ab) if len(ab) else None,
                                                  len(ab)))
        self.elections = ab

    def tally(self) -> None:
        """Tally every chain's current plan on the handle's stream, behind the runs already
        there (fw_chains_tally_async); no wait."""
        check(_lib.load().fw_chains_tally_async(self._h))

    def tally_info(self) -> dict:
        info = np.zeros(5, np.int64)
        check(_lib.load().fw_chains_tally_info(self._h, ptr(info)))
        return {"n_cols": int(info[0]), "n_elections": int(info[1]), "label_bits": int(info[2]),
                "n_groups": int(info[3]), "n_tallied": int(info[4]) + self._tally_base}

    def _read_tally(self, what, arr):
        check(_lib.load().fw_chains_read_tally(self._h, what, ptr(arr) if arr.size else None,
                                               arr.nbytes))
        return arr

    def tallies(self) -> np.ndarray:
        """int64 [n_chains, n_cols, k]: the district sums of every column, last tally."""
        n_cols = self.tally_info()["n_cols"]
        return self._read_tally(_lib.TALLY_SUMS, np.empty((self.n_chains, n_cols, self.k), np.int64))

    def seats(self) -> np.ndarray:
        """int32 [n_chains, n_elections, 2]: {districts the first column wins outright,
        districts tied} of the last tally."""
        n_el = self.tally_info()["n_elections"]
        return self._read_tally(_lib.TALLY_SEATS, np.empty((self.n_chains, n_el, 2), np.int32))

    def seat_hist(self) -> np.ndarray:
        """uint64 [n_groups, n_elections, k + 1]: tallied plans per seat count of the first
        column, over all tallies; one group, or one per rung under a ladder."""
        info = self.tally_info()
        return self._read_tally(_lib.TALLY_HIST, np.empty(
            (info["n_groups"], info["n_elections"], self.k + 1), np.uint64))

    def tally_reset(self) -> None:
        check(_lib.load().fw_chains_tally_reset(self._h))
        self._tally_base = 0

    # ------------------------------------------------------------- district geometry
    def set_geometry(self, edge_weights=None, area=None, exterior=None) -> None:
        """What the per-district geometry sums (fw_chains_set_geometry): integer
        ``edge_weights`` [n_edges] in ``Graph.edges()`` order (shared perimeters; None: every
        edge 1), ``area`` [n] (None: every node 1) and ``exterior`` [n], a node's exterior
        perimeter (None: 0).  Values >= 0, every total below 2^31 (``compactness.quantise``
        and ``Graph.edge_column`` make such arrays).  May be repeated: it replaces the arrays
        and zeroes the histogram and the count."""
        arrays = check_geometry_arrays(self.dgraph.n, self.dgraph.n_edges, edge_weights, area,
                                       exterior)
        check(_lib.load().fw_chains_set_geometry(self._h, *(ptr(a) for a in arrays)))
        self.geometry_arrays = arrays
        self._geometry_base = 0

    def geometry(self) -> None:
        """Measure every chain's current districts on the handle's stream, behind the runs
        already there (fw_chains_geometry_async); no wait."""
        check(_lib.load().fw_chains_geometry_async(self._h))

    def geometry_info(self) -> dict:
        info = np.zeros(5, np.int64)
        check(_lib.load().fw_chains_geometry_info(self._h, ptr(info)))
        return {"edge_weights": bool(info[0]), "label_bits": int(info[1]),
                "n_groups": int(info[2]), "n_edges": int(info[3]),
                "n_measured": int(info[4]) + self._geometry_base}

    def _read_geometry(self, what, arr):
        check(_lib.load().fw_chains_read_geometry(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def district_geometry(self) -> np.ndarray:
        """int64 [n_chains, k, 5] of the last measurement: per district {nodes, cut edges,
        interior perimeter, exterior perimeter, area}, the field indices ``compactness.NODES``
        .. ``compactness.AREA``."""
        return self._read_geometry(_lib.GEOM_DISTRICTS,
                                   np.empty((self.n_chains, self.k, 5), np.int64))

    def geometry_hist(self) -> np.ndarray:
        """uint64 [n_groups, n_edges + 1]: measured districts per cut-edge count, over all
        measurements; one group, or one per rung under a ladder."""
        info = self.geometry_info()
        return self._read_geometry(_lib.GEOM_HIST,
                                   np.empty((info["n_groups"], info["n_edges"] + 1), np.uint64))

    def geometry_reset(self) -> None:
        check(_lib.load().fw_chains_geometry_reset(self._h))
        self._geometry_base = 0

    # ------------------------------------------------------------- plan overlap and distance
    def set_reference(self, plans=None) -> None:
        """The plans ``overlap()`` compares with (fw_chains_set_reference).  ``None`` takes a
        snapshot of every chain's current plan on the handle's stream, behind the runs already
        there and with no wait; a 1-D plan [n] is shared by every chain; a 2-D array
        [n_chains, n] gives each chain its own.  Labels lie in [0, k); a reference need not be
        contiguous or balanced.  Replaces the reference and zeroes the distance histogram and
        the count."""
        if plans is None:
            check(_lib.load().fw_chains_set_reference(self._h, None, 0))
        else:
            a = np.asarray(plans)
            if a.dtype.kind not in "iu":
                raise ValueError(f"reference plans must be integers, got {a.dtype}")
            n = self.dgraph.n
            if a.shape != (n,) and a.shape != (self.n_chains, n):
                raise ValueError(f"reference plans must be [{n}] or [{self.n_chains}, {n}], "
                                 f"got {a.shape}")
            if a.size and (int(a.min()) < 0 or int(a.max()) >= self.k):
                raise ValueError(f"reference labels must lie in [0, {self.k})")
            a = np.ascontiguousarray(a, np.int16)
            check(_lib.load().fw_chains_set_reference(self._h, ptr(a), 1 if a.ndim == 2 else 0))
        self._overlap_base = 0

    def set_partners(self, partner=None) -> None:
        """The chain each chain is compared with by ``overlap("partner")``
        (fw_chains_set_partners): int [n_chains], default ``(c + 1) % n_chains``.  Two
        independent chains' overlap is the level a chain's overlap with its own past must
        reach at stationarity."""
        if partner is None:
            if self.n_chains < 2:
                raise ValueError("partners need at least two chains")
            partner = (np.arange(self.n_chains) + 1) % self.n_chains
        p = np.asarray(partner)
        if p.dtype.kind not in "iu" or p.shape != (self.n_chains,):
            raise ValueError(f"partner must be integers [{self.n_chains}]")
        if p.size and (int(p.min()) < 0 or int(p.max()) >= self.n_chains):
            raise ValueError(f"partners must lie in [0, {self.n_chains})")
        p = np.ascontiguousarray(p, np.int32)
        check(_lib.load().fw_chains_set_partners(self._h, ptr(p)))
        self.partners = p

    def overlap(self, against: str | int = "reference") -> None:
        """Compare every chain's current plan with its reference ("reference") or with its
        partner's current plan ("partner") on the handle's stream, behind the runs already
        there (fw_chains_overlap_async); no wait."""
        kind = OVERLAP_KINDS[against] if isinstance(against, str) else int(against)
        check(_lib.load().fw_chains_overlap_async(self._h, kind))

    def overlap_info(self) -> dict:
        info = np.zeros(5, np.int64)
        check(_lib.load().fw_chains_overlap_info(self._h, ptr(info)))
        return {"reference": ("none", "shared", "per_chain")[int(info[0])],
                "label_bits": int(info[1]), "n_groups": int(info[2]),
                "partners": bool(info[3]), "n_measured": int(info[4]) + self._overlap_base}

    def _read_overlap(self, what, arr):
        check(_lib.load().fw_chains_read_overlap(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def overlap_matrix(self) -> np.ndarray:
        """int64 [n_chains, k, k] of the last measurement: O[c, d, e] = nodes the reference
        labels d and the current plan labels e (``plandist`` turns it into scores)."""
        return self._read_overlap(_lib.OVERLAP_MATRIX,
                                  np.empty((self.n_chains, self.k, self.k), np.int64))

    def plan_distance(self) -> np.ndarray:
        """int32 [n_chains]: nodes labelled differently, last measurement."""
        return self._read_overlap(_lib.OVERLAP_DIST, np.empty(self.n_chains, np.int32))

    def distance_hist(self) -> np.ndarray:
        """uint64 [n_groups, n + 1]: measured plans per distance, over all measurements; one
        group, or one per rung under a ladder."""
        return self._read_overlap(_lib.OVERLAP_HIST, np.empty(
            (self.overlap_info()["n_groups"], self.dgraph.n + 1), np.uint64))

    def reference(self) -> np.ndarray:
        """int16 [n] (shared) or [n_chains, n]: the stored reference."""
        kind = self.overlap_info()["reference"]
        rows = self.n_chains if kind == "per_chain" else 1
        out = self._read_overlap(_lib.OVERLAP_REF, np.empty((rows, self.dgraph.n), np.int16))
        return out[0] if kind == "shared" else out

    def overlap_reset(self) -> None:
        check(_lib.load().fw_chains_overlap_reset(self._h))
        self._overlap_base = 0

    # ------------------------------------------------------------- ensemble census
    def enable_census(self, nodes: bool = True, edges: bool = True, boundary: bool = True) -> None:
        """Keep maps over the graph summed across the chains (fw_chains_enable_census): node
        occupancy per district (``nodes``), cut counts per edge (``edges``), boundary counts
        per node (``boundary``); under a ladder one set per rung.  Zeroes the arrays and the
        count; repeated, it replaces the previous set."""
        what = ((_lib.CENSUS_NODES if nodes else 0) | (_lib.CENSUS_EDGES if edges else 0) |
                (_lib.CENSUS_BOUNDARY if boundary else 0))
        if not what:
            raise ValueError("enable_census needs at least one of nodes, edges, boundary")
        check(_lib.load().fw_chains_enable_census(self._h, what))
        self._census_base = 0

    def census(self) -> None:
        """Add every chain's current plan to the enabled maps on the handle's stream, behind
        the runs already there (fw_chains_census_async); no wait."""
        check(_lib.load().fw_chains_census_async(self._h))

    def census_info(self) -> dict:
        info = np.zeros(5, np.int64)
        check(_lib.load().fw_chains_census_info(self._h, ptr(info)))
        what = int(info[0])
        return {"nodes": bool(what & _lib.CENSUS_NODES), "edges": bool(what & _lib.CENSUS_EDGES),
                "boundary": bool(what & _lib.CENSUS_BOUNDARY), "label_bits": int(info[1]),
                "n_groups": int(info[2]), "n_edges": int(info[3]),
                "n_measured": int(info[4]) + self._census_base}

    def _read_census(self, what, *shape):
        info = self.census_info()
        arr = np.empty((info["n_groups"],) + tuple(info[s] if isinstance(s, str) else s
                                                   for s in shape), np.uint64)
        check(_lib.load().fw_chains_read_census(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def node_occupancy(self) -> np.ndarray:
        """uint64 [n_groups, n, k]: chains that labelled node v with district d, over all
        censuses; one group, or one per rung under a ladder (``ensemble`` turns the arrays
        into frequencies and maps)."""
        return self._read_census(_lib.CENSUS_OCC, self.dgraph.n, self.k)

    def edge_cut_counts(self) -> np.ndarray:
        """uint64 [n_groups, n_edges]: chains that cut edge e (canonical ids: pairs u < w in
        CSR row order), over all censuses."""
        return self._read_census(_lib.CENSUS_ECUT, "n_edges")

    def boundary_counts(self) -> np.ndarray:
        """uint64 [n_groups, n]: chains in which node v had a neighbour of another district,
        over all censuses."""
        return self._read_census(_lib.CENSUS_BND, self.dgraph.n)

    def census_counts(self) -> np.ndarray:
        """uint64 [n_groups]: plans counted per group, over all censuses."""
        return self._read_census(_lib.CENSUS_CNT)

    def census_reset(self) -> None:
        check(_lib.load().fw_chains_census_reset(self._h))
        self._census_base = 0

    # ------------------------------------------------------------- node co-assignment
    def enable_coassignment(self, nodes=None) -> None:
        """Keep, summed across the chains, how many plans put nodes u and v in the same district
        (fw_chains_enable_coassign), for the distinct ``nodes`` in any order (``None``: all n);
        under a ladder one matrix per rung.  The handle takes the list sorted; every read comes
        back in the caller's order.  Zeroes the arrays and the count; repeated, it replaces the
        node list.  ``ValueError`` for duplicates."""
        if nodes is None:
            check(_lib.load().fw_chains_enable_coassign(self._h, None, 0))
            self._coassign_order = np.arange(self.dgraph.n)
        else:
            a = np.asarray(nodes).ravel()
            if a.size < 1 or a.dtype.kind not in "iu":
                raise ValueError("enable_coassignment: nodes must be a non-empty integer list")
            srt, inverse = np.unique(a, return_inverse=True)
            if srt.size != a.size:
                raise ValueError("enable_coassignment: duplicate nodes")
            srt = np.ascontiguousarray(srt, np.int32)
            check(_lib.load().fw_chains_enable_coassign(self._h, ptr(srt), srt.size))
            self._coassign_order = np.asarray(inverse).ravel()
        self._coassign_base = 0

    def coassign(self) -> None:
        """Add every chain's current plan to the co-assignment matrix on the handle's stream,
        behind the runs already there (fw_chains_coassign_async); no wait."""
        check(_lib.load().fw_chains_coassign_async(self._h))

    def coassign_info(self) -> dict:
        info = np.zeros(7, np.int64)
        check(_lib.load().fw_chains_coassign_info(self._h, ptr(info)))
        return {"m": int(info[0]), "label_bits": int(info[1]), "n_groups": int(info[2]),
                "n_measured": int(info[3]) + self._coassign_base, "tile": int(info[4]),
                "chunk": int(info[5]), "staged": bool(info[6])}

    def _read_coassign(self, what, arr):
        check(_lib.load().fw_chains_read_coassign(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def _coassign_perm(self, m):
        """The caller's order as positions in the handle's sorted list (a list the handle took
        some other way, a re-sized ladder's for one, reads in the handle's order)."""
        o = self._coassign_order
        return o if o is not None and o.size == m else np.arange(m)

    def coassignment(self) -> np.ndarray:
        """uint64 [n_groups, m, m]: plans of each group that put nodes i and j of the list (in
        the order given to ``enable_coassignment``) in one district, over all measurements;
        symmetric, the diagonal equal to ``coassign_counts()`` (``coassign`` turns it into
        frequencies, cores and entropies)."""
        info = self.coassign_info()
        m = max(info["m"], 1)
        t = self._read_coassign(_lib.COASSIGN_TOGETHER, np.empty((info["n_groups"], m, m), np.uint64))
        o = self._coassign_perm(m)
        return np.ascontiguousarray(t[:, o][:, :, o])

    def coassign_counts(self) -> np.ndarray:
        """uint64 [n_groups]: plans counted per group, over all measurements."""
        return self._read_coassign(_lib.COASSIGN_CNT,
                                   np.empty(self.coassign_info()["n_groups"], np.uint64))

    def coassign_nodes(self) -> np.ndarray:
        """int32 [m]: the node list, in the order given to ``enable_coassignment``."""
        m = max(self.coassign_info()["m"], 1)
        return self._read_coassign(_lib.COASSIGN_NODES, np.empty(m, np.int32))[self._coassign_perm(m)]

    def coassign_reset(self) -> None:
        check(_lib.load().fw_chains_coassign_reset(self._h))
        self._coassign_base = 0

    # ------------------------------------------------------------- pairwise plan distances
    def pair_distances(self, a=None, b=None) -> None:
        """Measure the Hamming distances between the current plans of the chains ``a`` and the
        chains ``b`` (member lists of chain ids, duplicates allowed; ``a=None``: all chains;
        ``b=None``: ``b = a``, the symmetric case) on the handle's stream, behind the runs
        already there (fw_chains_pairdist_async); no wait.  ``distance_matrix``,
        ``distance_rowsums`` and ``nearest_plans`` read the last measurement,
        ``pair_distance_hist`` the histogram over all of them."""
        if a is None:
            if b is None and self.n_chains ** 2 > _lib.PAIRDIST_MAX_PAIRS:
                raise ValueError(f"{self.n_chains} chains give more than 2^28 pairs: "
                                 "pass a member list")
            a = np.arange(self.n_chains, dtype=np.int32)
        a = np.ascontiguousarray(np.asarray(a).ravel(), np.int32)
        if b is None:
            check(_lib.load().fw_chains_pairdist_async(self._h, ptr(a), a.size, None, 0))
            return
        b = np.ascontiguousarray(np.asarray(b).ravel(), np.int32)
        if b.size < 1:
            raise ValueError("pair_distances: b is empty")
        check(_lib.load().fw_chains_pairdist_async(self._h, ptr(a), a.size, ptr(b), b.size))

    def pair_distance_info(self) -> dict:
        info = np.zeros(7, np.int64)
        check(_lib.load().fw_chains_pairdist_info(self._h, ptr(info)))
        return {"ma": int(info[0]), "mb": int(info[1]), "symmetric": bool(info[2]),
                "label_bits": int(info[3]), "n_measured": int(info[4]) + self._pairdist_base,
                "tile": int(info[5]), "chunk": int(info[6])}

    def _read_pairdist(self, what, arr):
        check(_lib.load().fw_chains_read_pairdist(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def distance_matrix(self) -> np.ndarray:
        """int32 [ma, mb]: D[i, j] = nodes at which the plans of chains a[i] and b[j] differ
        (districts by name), as of the last ``pair_distances``."""
        info = self.pair_distance_info()
        return self._read_pairdist(_lib.PAIRDIST_MATRIX,
                                   np.empty((max(info["ma"], 1), max(info["mb"], 1)), np.int32))

    def distance_rowsums(self) -> np.ndarray:
        """int64 [ma]: the row sums of ``distance_matrix()`` (``plancloud.medoid``)."""
        info = self.pair_distance_info()
        return self._read_pairdist(_lib.PAIRDIST_ROWSUM, np.empty(max(info["ma"], 1), np.int64))

    def nearest_plans(self) -> np.ndarray:
        """int32 [ma, 2]: per row the least distance and the lowest position j attaining it; in
        the symmetric case position i itself is left out ((-1, -1) for a single member)."""
        info = self.pair_distance_info()
        return self._read_pairdist(_lib.PAIRDIST_NEAREST,
                                   np.empty((max(info["ma"], 1), 2), np.int32))

    def pair_distance_hist(self) -> np.ndarray:
        """uint64 [n + 1]: counts of the measured distances over all ``pair_distances`` since
        the last reset: positions i < j in the symmetric case, every (i, j) otherwise."""
        return self._read_pairdist(_lib.PAIRDIST_HIST, np.empty(self.dgraph.n + 1, np.uint64))

    def pair_distance_reset(self) -> None:
        check(_lib.load().fw_chains_pairdist_reset(self._h))
        self._pairdist_base = 0

    # ------------------------------------------------------------- resampling across chains
    def clone(self, src) -> None:
        """Chain i continues from the current plan of chain ``src[i]`` (fw_chains_clone_async):
        int [n_chains], every value in [0, n_chains) and every source a fixed point
        (``src[src[i]] == src[i]``).  The plan moves (labels, populations, cut / bnodes / npairs
        / stuck, flagged-node counts, the current sampled wait, the family); the chain stays
        (its Philox counter, sums, counters, thr row, series).  Enqueued on the handle's stream
        behind the runs already there; no wait."""
        a = np.asarray(src)
        if a.dtype.kind not in "iu" or a.shape != (self.n_chains,):
            raise ValueError(f"src must be integers [{self.n_chains}]")
        a = np.ascontiguousarray(a, np.int32)
        check(_lib.load().fw_chains_clone_async(self._h, ptr(a)))

    def resample(self, base_from: float, base_to: float, round: Optional[int] = None) -> None:
        """One systematic resampling of the population for the change of base ``base_from`` ->
        ``base_to`` (fw_chains_resample_async with ``population.weight_table``): chains are
        re-weighted by (base_to / base_from) ** (-cut), the source map is drawn on the device and
        applied as ``clone``.  The draw is a function of (seed, chain_id0, round); ``round``
        defaults to ``resample_round``, which then advances.  No wait."""
        from .population import weight_table
        q, sign = weight_table(base_from, base_to, self.dgraph.n_edges)
        r = self.resample_round if round is None else int(round)
        check(_lib.load().fw_chains_resample_async(self._h, ptr(q), sign, r))
        self.resample_round = r + 1

    def resample_info(self) -> dict:
        """Waits for the stream; the counters and the integer sums of the last resample."""
        info = np.zeros(8, np.int64)
        check(_lib.load().fw_chains_resample_info(self._h, ptr(info)))
        return {"n_resampled": int(info[0]) + self._resample_base, "round": int(info[1]),
                "T": int(info[2]), "S2": int(info[3]), "cref": int(info[4]),
                "survivors": int(info[5]), "max_offspring": int(info[6]),
                "clones": int(info[7]) + self._clone_base}

    def _read_resample(self, what, dtype):
        arr = np.empty(self.n_chains, dtype)
        check(_lib.load().fw_chains_read_resample(self._h, what, ptr(arr), arr.nbytes))
        return arr

    def families(self) -> np.ndarray:
        """int32 [n_chains]: the chain whose initial plan each current plan descends from."""
        return self._read_resample(_lib.RESAMPLE_FAMILY, np.int32)

    def last_sources(self) -> np.ndarray:
        """int32 [n_chains]: the last map, of ``clone`` or ``resample``."""
        return self._read_resample(_lib.RESAMPLE_SRC, np.int32)

    def last_weights(self) -> np.ndarray:
        """uint32 [n_chains]: the weights of the last ``resample`` (the heaviest: 2^30)."""
        return self._read_resample(_lib.RESAMPLE_WEIGHTS, np.uint32)

    def run_annealed(self, bases, steps_per_stage: int, resample: bool = True,
                     record: bool = False, tally: bool = False, geometry: bool = False,
                     overlap: bool | str = False, max_retries: int = DEFAULT_MAX_RETRIES,
                     estimate: bool = True, census: bool = False, pairs=False,
                     coassign: bool = False):
        """Population annealing over ``bases``: at stage s every chain's bound table becomes
        that of ``bases[s]`` (a one-row ``set_schedule``, which stays in force afterwards), the
        population is resampled from ``bases[s - 1]`` (s >= 1, with ``resample``) and runs
        ``steps_per_stage`` steps; then tally, geometry, overlap, census, coassign, pairs (True: all
        chains, or a member list: one symmetric ``pair_distances``), record as asked.  The
        population is taken to sit at ``bases[0]`` on entry.  With ``estimate`` each stage's
        ``resample_info`` is read (one wait per stage) and the result is {"log_weight": the
        stages' ``population.log_weight_mean``, "log_z": their sum, "ess": the stages' effective
        sample sizes}; without it the resamples and runs are enqueued back to back, the tables'
        ``set_schedule`` calls being the only waits, and None is returned."""
        from .population import effective_sample_size, log_weight_mean
        bases = [float(b) for b in np.asarray(bases, np.float64).ravel()]
        D = self.dgraph.maxdeg
        logw, ess = [], []
        for s, b in enumerate(bases):
            self.set_schedule(metropolis_table(b, D)[None, :])
            if s and resample:
                self.resample(bases[s - 1], b)
                if estimate:
                    info = self.resample_info()
                    logw.append(log_weight_mean(info, bases[s - 1], b, self.n_chains))
                    ess.append(effective_sample_size(info))
            self.run_async(int(steps_per_stage), max_retries)
            if tally:
                self.tally()
            if geometry:
                self.geometry()
            if overlap:
                self.overlap("reference" if overlap is True else overlap)
            if census:
                self.census()
            if coassign:
                self.coassign()
            if pairs is not False and pairs is not None:
                self.pair_distances(None if pairs is True else pairs)
            if record:
                self.record()
        self.sync()
        if not (estimate and resample):
            return None
        return {"log_weight": np.array(logw), "log_z": float(np.sum(logw)), "ess": np.array(ess)}

    # ------------------------------------------------------------- sampled waits
    def enable_sampled_waits(self) -> None:
        """Draw geom_wait per state object (grid_chain_sec11.py:147-148, cached and re-used
        on re-yield) and sum it over yields (:368, :410-411); see fw_chains_enable_waits.
        Call before the first run."""
        pt = np.ascontiguousarray(wait_prob_table(self.dgraph.n, self.k))
        check(_lib.load().fw_chains_enable_waits(self._h, ptr(pt)))
        self.waits_on = True

    def waits(self) -> np.ndarray:
        """float64 [n_chains, 2]: {sum of the sampled waits over yields, the current
        state's draw}."""
        return self._read(_lib.READ_WAITS, np.empty((self.n_chains, 2), np.float64))

    def sampled_waits(self) -> np.ndarray:
        """Per chain, sum(waits) of grid_chain_sec11.py:410 (integer-valued floats)."""
        return self.waits()[:, 0].copy()

    # ------------------------------------------------------------- district shapes
    def enable_ring(self, ring_u, ring_w) -> None:
        """Count yields per pair of first two cut ring edges (boundary_slope and the
        driver's slope / angle, grid_chain_sec11.py:55-78,371-394); ``shape.ring_edges``
        builds the ring of a graph from the reference's predicates.  Zeroes the histogram.

        Parity holds for plans whose cut crosses the ring at most twice (k = 2 with both
        districts connected: the reference's sec11 and Frankenstein runs).  With more
        crossings the reference picks temp[0], temp[1] of ``list(set(...))`` (hash order),
        this handle the first two in ring order, so k > 2 shape histograms are not
        comparable with the reference's; a RuntimeWarning says so."""
        if self.k > 2:
            warnings.warn(f"enable_ring with k = {self.k}: plans can cut the ring more than "
                          "twice, where the pair kept (first two in ring order) differs from "
                          "the reference's set-order pick; shape parity holds for k = 2 only",
                          RuntimeWarning, stacklevel=2)
        u = np.ascontiguousarray(ring_u, np.int32)
        w = np.ascontiguousarray(ring_w, np.int32)
        if u.shape != w.shape or u.ndim != 1:
            raise ValueError("ring_u and ring_w must be equal-length 1-D arrays")
        check(_lib.load().fw_chains_enable_ring(self._h, ptr(u), ptr(w), len(u)))
        self.ring = (u, w)

    def hist_ring(self) -> np.ndarray:
        """uint64 [R*R+1]: yields per ring pair (i*R + j, i < j); [R*R]: fewer than two."""
        R = len(self.ring[0])
        return self._read(_lib.READ_HIST_RING, np.empty(R * R + 1, np.uint64))

    def ring_pairs(self) -> np.ndarray:
        """int32 [n_chains, 2]: each chain's current first two cut ring edges (-1: none)."""
        return self._read(_lib.READ_RING_PAIR, np.empty((self.n_chains, 2), np.int32))

    # ------------------------------------------------------------- checkpoint / resume
    def checkpoint(self) -> dict:
        """Everything a resumed chain needs: plans, the stats records (with the Philox
        attempt counter: the counter-based RNG makes resume exact) and the histograms; with
        a ladder set, also its bases, the placement, every chain's rung, the rung stats and
        the next round number."""
        ck = {"labels": self.labels(), "stats": self.stats(), "hist_cut": self.hist_cut(),
              "hist_b": self.hist_b(), "seed": np.uint64(self.seed),
              "chain_id0": np.int64(self.chain_id0), "thr": self.thr,
              "mode": np.int32(self.mode), "accept_rule": np.int32(self.accept_rule),
              "pop_lo": np.int64(self.pop_lo), "pop_hi": np.int64(self.pop_hi)}
        if self.node_flags is not None:
            ck["node_flags"] = self.node_flags
        if self._sched is not None:
            ck["sched_rows"], ck["sched_t0"] = self._sched, np.int64(self._sched_t0)
        if self.waits_on:
            ck["waits"] = self.waits()
        if getattr(self, "ring", None) is not None:
            ck["hist_ring"] = self.hist_ring()
            ck["ring_u"], ck["ring_w"] = self.ring
        if self.ladder_bases is not None:
            ck["ladder_bases"], ck["set_of_chain"] = self.ladder_bases, self.set_of_chain
            ck["rung"], ck["rung_stats"] = self.rungs(), self.rung_stats()
            ck["ladder_round"] = np.int64(self.ladder_round)
        if self.series_capacity:
            info = self.series_info()
            ck["series_capacity"] = np.int64(info["capacity"])
            for kind in ("cut", "bnodes", "rung"):
                ck["series_" + kind] = self.series(kind)
            # which samples' rung rows belong to the current ladder (the by-rung view)
            ck["series_valid"] = ((self._series_epoch[:info["n_samples"]] == info["epoch"]) &
                                  (info["epoch"] > 0))
        if self.columns is not None:
            ck["tally_columns"], ck["tally_elections"] = self.columns, self.elections
            if self.column_names is not None:
                ck["tally_names"] = np.array(self.column_names, dtype=np.str_)
            ck["tally_hist"] = self.seat_hist()
            ck["n_tallied"] = np.int64(self.tally_info()["n_tallied"])
        if self.geometry_arrays is not None:
            for key, a in zip(("geometry_edge_weights", "geometry_area", "geometry_exterior"),
                              self.geometry_arrays):
                if a is not None:
                    ck[key] = a
            ck["geometry_hist"] = self.geometry_hist()
            ck["n_measured"] = np.int64(self.geometry_info()["n_measured"])
        ovl = self.overlap_info()
        if ovl["reference"] != "none" or ovl["partners"]:
            if ovl["reference"] != "none":
                ck["overlap_reference"] = self.reference()
            if ovl["partners"]:
                ck["overlap_partners"] = self.partners
            ck["distance_hist"] = self.distance_hist()
            ck["n_overlaps"] = np.int64(ovl["n_measured"])
        rsm = self.resample_info()
        if rsm["clones"] or rsm["n_resampled"] or self.resample_round:
            ck["families"] = self.families()
            ck["n_resampled"], ck["n_clones"] = np.int64(rsm["n_resampled"]), np.int64(rsm["clones"])
            ck["resample_round"] = np.int64(self.resample_round)
        cen = self.census_info()
        if cen["nodes"] or cen["edges"] or cen["boundary"]:
            ck["census_parts"] = np.array([cen["nodes"], cen["edges"], cen["boundary"]], bool)
            ck["census_counts"] = self.census_counts()
            if cen["nodes"]:
                ck["census_occupancy"] = self.node_occupancy()
            if cen["edges"]:
                ck["census_edge_cut"] = self.edge_cut_counts()
            if cen["boundary"]:
                ck["census_boundary"] = self.boundary_counts()
            ck["n_censuses"] = np.int64(cen["n_measured"])
        pwd = self.pair_distance_info()
        if pwd["n_measured"]:
            ck["pair_distance_hist"] = self.pair_distance_hist()
            ck["n_pair_distances"] = np.int64(pwd["n_measured"])
        coa = self.coassign_info()
        if coa["m"]:
            ck["coassign_nodes"] = self.coassign_nodes()
            ck["coassign_together"] = self.coassignment()
            ck["coassign_counts"] = self.coassign_counts()
            ck["n_coassigned"] = np.int64(coa["n_measured"])
        return ck

    def restore(self, ck: dict) -> None:
        """Load a ``checkpoint`` into this handle (same graph, chain count, seed and chain
        ids): the chains continue exactly where the checkpointed ones stopped."""
        if int(ck["seed"]) != self.seed or int(ck["chain_id0"]) != self.chain_id0:
            raise ValueError("checkpoint of another seed / chain-id range")
        if "mode" in ck and int(ck["mode"]) != self.mode:
            raise ValueError(f"checkpoint of proposal mode {int(ck['mode'])}, handle has "
                             f"{self.mode}")
        if "pop_lo" in ck and (int(ck["pop_lo"]), int(ck["pop_hi"])) != (self.pop_lo, self.pop_hi):
            raise ValueError(f"checkpoint of population bounds [{int(ck['pop_lo'])}, "
                             f"{int(ck['pop_hi'])}], handle has [{self.pop_lo}, {self.pop_hi}]")
        if self.waits_on and "waits" not in ck:
            raise ValueError("sampled waits are enabled but the checkpoint carries none: the "
                             "resumed sums would miss every earlier yield")
        L = _lib.load()
        if "waits" in ck and not self.waits_on:
            self.enable_sampled_waits()
        for what, key in ((_lib.READ_LABELS, "labels"), (_lib.READ_STATS, "stats"),
                          (_lib.READ_HIST_CUT, "hist_cut"), (_lib.READ_HIST_B, "hist_b")):
            a = np.ascontiguousarray(ck[key])
            if key == "stats":
                a = np.ascontiguousarray(a, STATS_DTYPE)
                if a.shape != (self.n_chains,):
                    raise ValueError("checkpoint of another chain count")
            check(L.fw_chains_write(self._h, what, ptr(a), a.nbytes))
        if "waits" in ck:
            a = np.ascontiguousarray(ck["waits"], np.float64)
            check(L.fw_chains_write(self._h, _lib.READ_WAITS, ptr(a), a.nbytes))
        if "hist_ring" in ck:
            self.enable_ring(ck["ring_u"], ck["ring_w"])
            a = np.ascontiguousarray(ck["hist_ring"], np.uint64)
            check(L.fw_chains_write(self._h, _lib.READ_HIST_RING, ptr(a), a.nbytes))
        # the accept rule and the bound schedule the checkpointed chains ran under (after the
        # plans: the boundary rule's flagged-node counts are taken from them)
        if "accept_rule" in ck:
            rule, fl = int(ck["accept_rule"]), ck.get("node_flags")
            same = rule == self.accept_rule and (
                (fl is None and self.node_flags is None) or
                (fl is not None and self.node_flags is not None and
                 np.array_equal(np.asarray(fl, np.uint8), self.node_flags)))
            # the labels write above already re-derived the boundary rule's flagged-node
            # counts for the handle's own flags; only a different rule or flag set needs them
            # recounted
            if not same:
                self.set_accept(rule, fl)
        if "sched_rows" in ck:
            self.set_schedule(ck["sched_rows"], int(ck["sched_t0"]))
        elif "accept_rule" in ck:
            self.set_schedule(None)
        # the ladder last: it snapshots the stats records written above, and every chain
        # takes the bounds of the rung it had reached
        if "ladder_bases" in ck:
            self.set_ladder(ck["ladder_bases"], ck["set_of_chain"], ck["rung"])
            a = np.ascontiguousarray(ck["rung_stats"])
            if a.nbytes != self.n_chains * _lib.RUNG_STATS_DTYPE.itemsize:
                raise ValueError("checkpoint of another ladder shape")
            check(L.fw_chains_write(self._h, _lib.READ_RUNG_STATS, ptr(a), a.nbytes))
            self.ladder_round = int(ck["ladder_round"])
        # the series after the ladder: rung rows are checked against, and stamped with, it.
        # Rung rows recorded under an earlier ladder are not carried (they read as -1).
        if "series_capacity" in ck:
            cut = np.ascontiguousarray(ck["series_cut"], np.int32)
            if not self.series_capacity:
                self.enable_series(int(ck["series_capacity"]))
            elif self.series_capacity < cut.shape[0]:
                raise ValueError(f"checkpoint of {cut.shape[0]} samples, handle holds "
                                 f"{self.series_capacity}")
            self.series_reset()
            if cut.shape[0]:
                self.write_series("cut", cut)
                self.write_series("bnodes", ck["series_bnodes"])
                valid = np.asarray(ck["series_valid"], bool)
                edges = np.flatnonzero(np.diff(np.r_[False, valid, False].astype(np.int8)))
                for lo, hi in zip(edges[::2], edges[1::2]):
                    self.write_series("rung", ck["series_rung"][lo:hi], t0=int(lo))
        # the tally after the ladder as well: set_ladder zeroes the seat histogram, whose
        # shape follows the rung count
        if "tally_columns" in ck:
            cols = np.asarray(ck["tally_columns"])
            if "tally_names" in ck:
                cols = {str(name): col for name, col in zip(ck["tally_names"], cols)}
            self.set_columns(cols)
            self.set_elections(np.asarray(ck["tally_elections"], np.int32).reshape(-1, 2))
            hist = np.ascontiguousarray(ck["tally_hist"], np.uint64)
            if hist.shape != self.seat_hist().shape:
                raise ValueError("checkpoint of another seat histogram shape")
            check(L.fw_chains_write_tally(self._h, _lib.TALLY_HIST,
                                          ptr(hist) if hist.size else None, hist.nbytes))
            self._tally_base = int(ck["n_tallied"]) - (self.tally_info()["n_tallied"] -
                                                       self._tally_base)
        # the geometry after the ladder too: set_ladder re-sizes its histogram by rung
        if "geometry_hist" in ck:
            self.set_geometry(*(np.asarray(ck[key]) if key in ck else None for key in
                                ("geometry_edge_weights", "geometry_area", "geometry_exterior")))
            hist = np.ascontiguousarray(ck["geometry_hist"], np.uint64)
            if hist.shape != self.geometry_hist().shape:
                raise ValueError("checkpoint of another geometry histogram shape")
            check(L.fw_chains_write_geometry(self._h, _lib.GEOM_HIST, ptr(hist), hist.nbytes))
            self._geometry_base = int(ck["n_measured"])  # set_geometry zeroed the handle's count
        # and the overlap: its histogram is kept by rung as well
        if "distance_hist" in ck:
            if "overlap_reference" in ck:
                self.set_reference(np.asarray(ck["overlap_reference"]))
            if "overlap_partners" in ck:
                self.set_partners(np.asarray(ck["overlap_partners"]))
            hist = np.ascontiguousarray(ck["distance_hist"], np.uint64)
            if hist.shape != self.distance_hist().shape:
                raise ValueError("checkpoint of another distance histogram shape")
            check(L.fw_chains_write_overlap(self._h, _lib.OVERLAP_HIST, ptr(hist), hist.nbytes))
            # the handle's own count went on unless a reference was set just now
            self._overlap_base = int(ck["n_overlaps"]) - (self.overlap_info()["n_measured"] -
                                                          self._overlap_base)
        # the families and the resample counters (the handle's own counts went on)
        if "families" in ck:
            a = np.ascontiguousarray(ck["families"], np.int32)
            if a.shape != (self.n_chains,):
                raise ValueError("checkpoint of another chain count")
            check(L.fw_chains_write_resample(self._h, _lib.RESAMPLE_FAMILY, ptr(a), a.nbytes))
            now = self.resample_info()
            self._resample_base += int(ck["n_resampled"]) - now["n_resampled"]
            self._clone_base += int(ck["n_clones"]) - now["clones"]
            self.resample_round = int(ck["resample_round"])
        # the census after the ladder: its arrays are kept by rung
        if "census_parts" in ck:
            self.enable_census(*(bool(x) for x in np.asarray(ck["census_parts"])))
            for what, key in ((_lib.CENSUS_CNT, "census_counts"),
                              (_lib.CENSUS_OCC, "census_occupancy"),
                              (_lib.CENSUS_ECUT, "census_edge_cut"),
                              (_lib.CENSUS_BND, "census_boundary")):
                if key in ck:
                    a = np.ascontiguousarray(ck[key], np.uint64)
                    check(L.fw_chains_write_census(self._h, what, ptr(a), a.nbytes))
            self._census_base = int(ck["n_censuses"])  # enable_census zeroed the handle's count
        if "pair_distance_hist" in ck:
            hist = np.ascontiguousarray(ck["pair_distance_hist"], np.uint64)
            if hist.shape != (self.dgraph.n + 1,):
                raise ValueError(f"pair_distance_hist has shape {hist.shape}, the handle's is "
                                 f"{(self.dgraph.n + 1,)}")
            check(L.fw_chains_write_pairdist(self._h, _lib.PAIRDIST_HIST, ptr(hist), hist.nbytes))
            self._pairdist_base = int(ck["n_pair_distances"]) - (
                self.pair_distance_info()["n_measured"] - self._pairdist_base)
        # the co-assignment after the ladder as well: its matrices are kept by rung.  The
        # checkpoint holds the caller's order; the handle's is the sorted one.
        if "coassign_nodes" in ck:
            self.enable_coassignment(np.asarray(ck["coassign_nodes"]))
            o = np.argsort(self._coassign_order)  # sorted position -> caller's position
            t = np.ascontiguousarray(np.asarray(ck["coassign_together"], np.uint64)[:, o][:, :, o])
            cnt = np.ascontiguousarray(ck["coassign_counts"], np.uint64)
            info = self.coassign_info()
            if t.shape != (info["n_groups"], info["m"], info["m"]) or cnt.shape != (info["n_groups"],):
                raise ValueError("checkpoint of another co-assignment shape")
            check(L.fw_chains_write_coassign(self._h, _lib.COASSIGN_TOGETHER, ptr(t), t.nbytes))
            check(L.fw_chains_write_coassign(self._h, _lib.COASSIGN_CNT, ptr(cnt), cnt.nbytes))
            self._coassign_base = int(ck["n_coassigned"])  # enable zeroed the handle's count

    def save_checkpoint(self, path: str) -> None:
        ck = self.checkpoint()
        ck["stats"] = ck["stats"].view(np.uint8)  # plain bytes: loadable without pickle
        if "rung_stats" in ck:
            ck["rung_stats"] = ck["rung_stats"].view(np.uint8)
        np.savez(path, **ck)

    @classmethod
    def from_checkpoint(cls, dgraph: "DeviceGraph", path: str, k: int, proposal=None,
                        pop_bounds=None, percent: float = 0.05) -> "Chains":
        """A new handle resumed from ``save_checkpoint`` output (numpy, no pickle), with the
        proposal mode, population bounds, accept rule and bound schedule the checkpointed
        chains ran under (``pop_bounds`` / ``percent`` only for checkpoints without bounds)."""
        d = np.load(path, allow_pickle=False)
        labels = d["labels"]
        if proposal is None:
            proposal = int(d["mode"]) if "mode" in d.files else "pairs"
        if pop_bounds is None and "pop_lo" in d.files:
            pop_bounds = (int(d["pop_lo"]), int(d["pop_hi"]))
        ch = cls(dgraph, labels.shape[0], k, labels, proposal=proposal, pop_bounds=pop_bounds,
                 percent=percent, seed=int(d["seed"]), chain_id0=int(d["chain_id0"]),
                 thr=d["thr"])
        ck = {key: d[key] for key in d.files}
        ck["stats"] = d["stats"].view(STATS_DTYPE)
        ch.restore(ck)
        return ch

    # ------------------------------------------------------------- spatial maps
    def enable_maps(self, label_values: Optional[Sequence[int]] = None) -> None:
        """Track the reference driver's per-edge / per-node maps on every chain
        (grid_chain_sec11.py:383-384, 396-400).  ``label_values``: the GerryChain
        assignment value of each district index (default 0..k-1; {-1, 1} for the
        reference's k=2 plans).  Call before the first run."""
        lv = None
        if label_values is not None:
            lv = np.ascontiguousarray(label_values, np.int64)
            if len(lv) != self.k:
                raise ValueError(f"need {self.k} label values")
        check(_lib.load().fw_chains_enable_maps(self._h, ptr(lv)))
        self.label_values = (np.arange(self.k, dtype=np.int64) if lv is None else lv)

    MAPS = {"cut_times": _lib.MAP_CUT_TIMES, "num_flips": _lib.MAP_NUM_FLIPS,
            "part_sum": _lib.MAP_PART_SUM, "last_flipped": _lib.MAP_LAST_FLIPPED}

    def read_map(self, what: str, chains=None, total: bool = False,
                 finalize: bool = False) -> np.ndarray:
        """int64 map ``what`` (cut_times [E], num_flips / part_sum / last_flipped [n]) of
        chains ``range(*chains)`` (default all) as [n_chains, len], or summed over them
        (``total``).  ``finalize`` applies grid_chain_sec11.py:416-419 to part_sum."""
        lo, hi = (0, self.n_chains) if chains is None else (int(chains[0]), int(chains[1]))
        m = self.dgraph.n_edges if what == "cut_times" else self.dgraph.n
        out = np.empty(m if total else (hi - lo, m), np.int64)
        flags = (_lib.MAP_SUM if total else 0) | (_lib.MAP_FINALIZE if finalize else 0)
        check(_lib.load().fw_chains_read_map(self._h, self.MAPS[what], lo, hi - lo, flags,
                                             ptr(out), out.nbytes))
        return out

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            _lib.load().fw_chains_destroy(h)
            h.value = None  # the handle object is shared with DeviceGraph._live
            self.dgraph._live.pop(id(h), None)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_flips(dgraph: DeviceGraph, labels, k: int, v, target, pop_bounds):
    """Batched per-flip verdicts on one state (fw_eval_flips)."""
    L = _lib.require_device()
    lab = np.ascontiguousarray(labels, np.int16)
    v = np.ascontiguousarray(v, np.int32)
    t = np.ascontiguousarray(target, np.int16)
    m = len(v)
    dcut = np.zeros(m, np.int32)
    contig = np.zeros(m, np.uint8)
    pop_ok = np.zeros(m, np.uint8)
    db = np.zeros(m, np.int32)
    check(L.fw_eval_flips(dgraph.handle, ptr(lab), int(k), ptr(v), ptr(t), m, int(pop_bounds[0]),
                          int(pop_bounds[1]), ptr(dcut), ptr(contig), ptr(pop_ok), ptr(db)))
    return dcut, contig, pop_ok, db


@dataclass
class RunResult:
    labels: np.ndarray      # [n_chains, n] final plans
    stats: np.ndarray       # [n_chains] STATS_DTYPE
    hist_cut: np.ndarray    # yields per |cut edges|
    hist_b: np.ndarray      # yields per |B|
    pops: np.ndarray        # [n_chains, k]
    kernel_ms: float
    maps: Optional[dict] = None  # spatial observables (Chains.read_map), per chain
    waits: Optional[np.ndarray] = None  # sampled geom_wait sums per chain (Chains.sampled_waits)

    def expected_wait_sums(self, n_nodes: int, k: int) -> np.ndarray:
        return expected_wait_sum(self.stats, n_nodes, k)


def read_maps(ch: "Chains", finalize: bool = True) -> dict:
    """All four spatial maps of every chain; part_sum finalised as the reference's
    end-of-run loop does (grid_chain_sec11.py:416-419) unless ``finalize`` is False."""
    return {"cut_times": ch.read_map("cut_times"), "num_flips": ch.read_map("num_flips"),
            "part_sum": ch.read_map("part_sum", finalize=finalize),
            "last_flipped": ch.read_map("last_flipped")}


def run_chains(graph: Graph, init_labels, k: int, n_chains: int, steps: int,
               proposal: str | int = "pairs", percent: float = 0.05, base=1.0, seed: int = 0,
               chain_id0: int = 0, device: int = 0, pop_bounds=None,
               max_retries: int = DEFAULT_MAX_RETRIES, total_steps: Optional[int] = None,
               maps: bool = False, label_values=None, waits: bool = False) -> RunResult:
    """Run ``n_chains`` chains for ``steps`` counted steps each and read everything back.

    ``total_steps`` (GerryChain's meaning: yields including the initial state) may be
    given instead of ``steps``; then steps = total_steps - 1.  ``maps`` also returns the
    driver's spatial observables (``label_values``: GerryChain values of districts 0..k-1);
    ``waits`` the sampled geom_wait sums (grid_chain_sec11.py:147-148,410-411).
    """
    if total_steps is not None:
        steps = int(total_steps) - 1
    dg = DeviceGraph(graph, device)
    ch = Chains(dg, n_chains, k, init_labels, proposal=proposal, pop_bounds=pop_bounds,
                percent=percent, base=base, seed=seed, chain_id0=chain_id0)
    if maps:
        ch.enable_maps(label_values)
    if waits:
        ch.enable_sampled_waits()
    ch.run(steps, max_retries)
    res = RunResult(ch.labels(), ch.stats(), ch.hist_cut(), ch.hist_b(), ch.pops(),
                    ch.last_kernel_ms(), read_maps(ch) if maps else None,
                    ch.sampled_waits() if waits else None)
    ch.close()
    dg.close()
    return res
