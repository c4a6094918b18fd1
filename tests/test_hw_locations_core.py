"""CPU: the ENDS mode of hw_run and the per-end START pass (csrc/hw_core.hpp) through the tile emulator tests/emul/hw_loc_emul.cpp (plain
g++ build) on the designed tiles of tests/hw_locations_cases.py: counts, ends and starts equal the plain restatement for every window
width W = 1, 2, 4, 8 that holds the tile's band, and a width that does not hold it says so."""
import ctypes
import os
import subprocess

import pytest

import hw_locations_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_hw_loc_emul.so")
SRC = os.path.join(HERE, "emul", "hw_loc_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_core.hpp")]
WIDTHS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def run_tile(L, WE, WS, q, targets, hs, cap):
    n = len(targets)
    arr = (ctypes.c_char_p * n)(*[t.encode() for t in targets])
    tl = (ctypes.c_int * n)(*[len(t) for t in targets])
    hh = (ctypes.c_int * n)(*hs)
    cnt = (ctypes.c_int32 * n)()
    ends = (ctypes.c_int32 * (cap * n))(*([-7] * (cap * n)))
    starts = (ctypes.c_int32 * (cap * n))(*([-7] * (cap * n)))
    L.emul_hw_loc_tile(WE, WS, q.encode(), len(q), n, arr, tl, hh, cap, cnt, ends, starts)
    return [(cnt[i], [(starts[cap * i + c], ends[cap * i + c]) for c in range(max(0, min(cnt[i], cap)))]) for i in range(n)]


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_emulator_equals_the_restatement(emul, group):
    exp = C.expected(group)
    tiles = fits = 0
    for c in C.cases(group):
        P = len(c.query)
        for W0, idx in C.ends_tiles(c, group):
            hs = [exp[c.name, i][0] for i in idx]
            targets = [c.targets[i] for i in idx]
            cap = max(len(exp[c.name, i][1]) for i in idx)
            band = C.rows(max(len(t) - P for t in targets), max(hs))
            assert C.words(band) == W0
            tiles += 1
            for WE in WIDTHS:
                WS0 = C.words(2 * max(hs) + 1)
                for WS in ([w for w in WIDTHS if w >= WS0] if WE == W0 else [WS0]):
                    got = run_tile(emul, WE, WS, c.query, targets, hs, cap)
                    if band > 64 * WE:
                        assert all(g[0] == -3 for g in got), (c.name, WE)
                        continue
                    fits += 1
                    for i, g in zip(idx, got):
                        assert g == (len(exp[c.name, i][1]), list(exp[c.name, i][1])), (c.name, i, WE, WS, g[0], g[1][:3], exp[c.name, i][1][:3])
                if WE == W0 and WS0 > 1:          # a START window too narrow for the tile's largest distance
                    got = run_tile(emul, WE, WS0 // 2, c.query, targets, hs, cap)
                    assert all(s == -3 for g in got for s, e in g[1]) and [g[0] for g in got] == [len(exp[c.name, i][1]) for i in idx]
    assert tiles >= 1 and fits > tiles


def test_threshold_above_the_distance_finds_no_end_and_below_none(emul):
    """ENDS reports the columns that EQUAL ln.h: with a lane's threshold one above its distance the columns it reports are those of value
    h + 1 (never those of h), and a lane that is no hit (h < 0) stays empty"""
    c, = [c for c in C.cases("c") if c.name == "c_exact_x2"]
    t = c.targets[0]
    last = C._last_row(c.query, t, True)[1:]
    got = run_tile(emul, 1, 1, c.query, [t, t, t], [0, 1, -1], len(t))
    assert [e for s, e in got[0][1]] == [j for j in range(len(t)) if last[j] == 0] and got[0][0] == 2
    assert [e for s, e in got[1][1]] == [j for j in range(len(t)) if last[j] == 1 and j + 1 >= len(c.query) - 1]
    assert got[2] == (0, [])
