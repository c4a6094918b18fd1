"""CPU: the PREFIX_LOCATE and PREFIX_ENDS modes of hw_run (csrc/hw_core.hpp) and the prefix cut rule (csrc/hw_plan.hpp) through the tile
emulator tests/emul/shw_emul.cpp (plain g++ build) on the designed cases of tests/shw_cases.py: distance, first end, end count and every
end equal the plain restatement for every window width W = 1, 2, 4, 8 that holds the tile's band, and a width that does not hold it
says so (-3)."""
import ctypes
import os
import subprocess

import pytest

import shw_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_shw_emul.so")
SRC = os.path.join(HERE, "emul", "shw_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_core.hpp", "hw_plan.hpp")]
WIDTHS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def run_query(L, W, q, targets, thr, cap):
    """[(h, first end, count, [ends], words of the LOCATE tile)] per target; thr < 0: the pair takes no part"""
    n = len(targets)
    arr = (ctypes.c_char_p * n)(*[t.encode() for t in targets])
    tl = (ctypes.c_int * n)(*[len(t) for t in targets])
    th = (ctypes.c_int * n)(*thr)
    h, end, cnt, w = ((ctypes.c_int32 * n)() for _ in range(4))
    ends = (ctypes.c_int32 * (cap * n))(*([-7] * (cap * n)))
    L.emul_shw_query(W, q.encode(), len(q), n, arr, tl, th, cap, h, end, cnt, ends, w)
    return [(h[i], end[i], cnt[i], [ends[cap * i + c] for c in range(max(0, min(cnt[i], cap)))], w[i]) for i in range(n)]


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_emulator_equals_the_restatement(emul, group):
    exp = C.expected(group)
    fits = narrow = 0
    for c in C.cases(group):
        P = len(c.query)
        # the threshold each pair settles under (the driver's clamp and rounds, restated)
        thr = [min(C.clamp(k, P), C.ROUND_THR[l["round"]]) for k, l in zip(c.ks, c.lanes)]
        cap = max(1, max(len(exp[c.name, i][1]) for i in range(len(c.targets))))
        for W in WIDTHS:
            got = run_query(emul, W, c.query, list(c.targets), thr, cap)
            for i, (g, t) in enumerate(zip(got, c.targets)):
                ed, ends = exp[c.name, i]
                if not C.needs_kernel(P, len(t), thr[i]):
                    assert g == (-1, -1, 0, [], 0) and ed == -1, (c.name, i, W, g)
                    continue
                assert g[4] == C.words(2 * thr[i] + 1) == c.lanes[i]["words"], (c.name, i, g[4])
                if g[4] > W:          # the tile's band does not fit: said so, nothing else
                    assert g[:4] == (-3, -1, 0, []), (c.name, i, W, g)
                    narrow += 1
                    continue
                fits += 1
                if ed < 0:
                    assert g[:4] == (-1, -1, 0, []), (c.name, i, W, g)
                else:
                    # (an ENDS tile of distances h <= thr is never wider than the LOCATE tile)
                    assert g[:4] == (ed, ends[0], len(ends), list(ends)), (c.name, i, W, g[:3], g[3][:4], ed, ends[:4])
    assert fits > 0 and (narrow > 0 or group in "bcd")


def test_rounds_below_the_settling_one_miss(emul):
    """group e's pairs under the thresholds of the rounds BEFORE the one that settles them: every one a miss there, as the driver needs"""
    c, = C.cases("e")
    for r, cap_thr in enumerate(C.ROUND_THR[:3]):
        idx = [i for i, l in enumerate(c.lanes) if l["round"] > r]
        got = run_query(emul, 8, c.query, [c.targets[i] for i in idx], [cap_thr] * len(idx), 1)
        assert idx and all(g[:4] == (-1, -1, 0, []) for g in got), (r, got)
    q, far = C.far_pair()
    assert run_query(emul, 8, q, [far], [255], 1)[0][:4] == (-1, -1, 0, [])


def test_mixed_thresholds_share_a_tile_and_threshold_selects(emul):
    """one target under thresholds h - 1, h, h + 5 in one tile: a miss, a hit and a hit, the ends of the hits alike (ENDS runs on h)"""
    c, = [c for c in C.cases("c") if c.name == "c_a20"]
    t = c.targets[0]
    got = run_query(emul, 1, c.query, [t, t, t, t], [9, 10, 15, -1], 16)
    assert got[0][:4] == (-1, -1, 0, []) and got[1][:4] == got[2][:4] == (10, 9, 11, list(range(9, 20))) and got[3] == (-1, -1, 0, [], 0)


def test_random_list_through_the_emulator(emul):
    seqs, q, t, k = C.random_list()
    by_q = {}
    for p in range(0, len(q), 3):
        by_q.setdefault(q[p], []).append(p)
    checked = 0
    for qi, ps in by_q.items():
        P = len(seqs[qi])
        thr = [min(C.clamp(k[p], P), 255) for p in ps]
        exp = [C.restated_cached(seqs[qi], seqs[t[p]], thr_p) for p, thr_p in zip(ps, thr)]
        cap = max(1, max(len(e[1]) for e in exp))
        got = run_query(emul, 8, seqs[qi], [seqs[t[p]] for p in ps], thr, cap)
        for g, e in zip(got, exp):
            assert g[:4] == ((e[0], e[1][0], len(e[1]), list(e[1])) if e[0] >= 0 else (-1, -1, 0, [])), (qi, g[:3], e[0], e[1][:3])
            checked += 1
    assert checked > 600
