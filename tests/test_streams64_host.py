"""The oracle's draw layout, pinned once against the mapping include/flipwalk.h documents.

A pure-Python Philox4x32-10 (checked against the Random123 known-answer vectors that
tests/test_oracle.py uses) replays the first counted steps of one chain on the 4 x 4 grid by
hand, at a (seed, chain id, attempt) whose three high words are all non-zero:
key = (lo32(seed), hi32(seed)), counter = (lo32(attempt), hi32(attempt), lo32(chain),
hi32(chain)); the proposal is element floor(((x1 << 32) | x0) * P / 2^64) of the proposal set
in canonical order; u = ((x2 >> 5) * 2^26 + (x3 >> 6)) * 2^-53.  Validity and the accept bound
come from law_ref, not from the oracle.
"""
import numpy as np
import pytest

import law_cases as LC
from cases import MU
from oracle import oracle as O

M32 = 0xFFFFFFFF
KAT = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
       ([M32] * 4, [M32] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
       ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_python_philox_known_answers(ctr, key, out):
    assert philox4x32_10(ctr, key) == out


SEED, CHAIN, ATTEMPT0 = 0x9E3779B97F4A7C15, 2**40 + 3, 2**33 + 2**32 - 2


@pytest.mark.parametrize("mode", ["pairs", "cutedge"])
@pytest.mark.parametrize("si", [1, 2])
def test_oracle_draws_follow_the_documented_mapping(mode, si):
    """Three counted steps (at least three attempts, the attempt counter carrying into its
    high word on the way) replayed by hand; after each the oracle's plan and counters must agree."""
    g, k, (lo, hi), _, _ = LC.graph_case("g4x4")
    L = LC.chain_law("g4x4", mode, MU)
    thr = LC.thr_table("g4x4", MU)
    plan = LC.start_plans("g4x4")[si]
    want = {"attempts": ATTEMPT0, "steps": 0, "accepts": 0, "pop_fail": 0, "contig_fail": 0}
    st = O.new_stats(1)
    st["attempts"], st["yields"] = ATTEMPT0, 1  # a resumed chain: no initial yield
    lab = np.array(plan, np.int16)
    for _ in range(3):
        while True:  # attempts until a valid proposal
            # canonical order: nodes ascending; distinct foreign labels ascending (pairs) or
            # the node's foreign neighbours in ascending node order (cutedge)
            props = L.proposals(plan)
            order = []
            for p in props:
                v, b, w = p[0], p[1], p[2]
                if mode == "pairs":
                    order.append((v, b, p))
                else:
                    order += [(v, u, p) for u in L.nbrs[v] if plan[u] == b]
            if mode == "cutedge":
                order.sort(key=lambda e: (e[0], e[1]))
            a = want["attempts"]
            x = philox4x32_10([a & M32, a >> 32, CHAIN & M32, CHAIN >> 32],
                              [SEED & M32, SEED >> 32])
            want["attempts"] += 1
            rank = (((x[1] << 32) | x[0]) * len(order)) >> 64
            v, _, p = order[rank]
            if p[3] == "pop":
                want["pop_fail"] += 1
            elif p[3] == "contig":
                want["contig_fail"] += 1
            else:
                break
        want["steps"] += 1
        u = ((x[2] >> 5) * 67108864 + (x[3] >> 6)) / 9007199254740992
        if u < MU ** (-p[4]):
            want["accepts"] += 1
            plan = p[5]
        lab, st, _, _ = O.run_chain(g, lab, k, LC.MODE_ID[mode], lo, hi, thr, SEED, CHAIN, 1,
                                    stats=st)
        assert tuple(int(z) for z in lab) == plan
        for f, value in want.items():
            assert int(st[f][0]) == value, (f, int(st[f][0]), value)
    assert ATTEMPT0 >> 32 == 2 and want["attempts"] >> 32 == 3  # the carry was taken
