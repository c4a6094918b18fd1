"""CPU: the designed inputs of the banded infix kernels (tests/hw_edge_cases.py) have the properties they were built for -- every claim
of every lane against the oracle's full matrices (hw_locate + nw_path), coverage totals per group so that an edit of the generator cannot
silently empty one -- and the tile emulator (tests/emul/hw_emul.cpp on csrc/hw_core.hpp, plain g++ build) gives the oracle's rows on the
tiles the host's greedy cut forms from them."""
import ctypes
import os
import subprocess

import pytest

import hw_edge_cases as E
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_hw_emul.so")
SRC = os.path.join(HERE, "emul", "hw_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_core.hpp")]
MISS = E.MISS


def restated_rows(delta, k):
    """csrc/hw_core.hpp hw_locate_rows"""
    return (delta if delta > 0 else 0) + 2 * k + 1


oracle_rows = E.oracle_rows


def check_lane(c, i, row):
    q, t, k, claim = c.query, c.targets[i], c.ks[i], c.lanes[i]
    where = (c.name, i, claim, row)
    delta = len(t) - len(q)
    assert E.rows(delta, k) == restated_rows(delta, k)
    if "rows" in claim:
        assert restated_rows(delta, k) == claim["rows"], where
    if "own_w" in claim:
        assert E.words(restated_rows(delta, k)) == claim["own_w"], where
    if "fin_w" in claim:
        assert E.words(2 * k + 1) == claim["fin_w"], where
    if "dist" in claim:
        assert O.hw_locate(q, t, -1)[0] == claim["dist"], where
        if claim["dist"] > k:
            assert row == MISS, where
            return
        assert row[0] == claim["dist"], where
    if row[0] < 0:
        return
    for key, got in (("start", row[1]), ("end", row[2]), ("lead", row[3]), ("trail", row[4]), ("ms", row[2] - row[1] + 1)):
        if key in claim:
            assert got == claim[key], (key,) + where
    if row[1] > 0:
        assert row[3] == 0, where                         # (only start == 0 has a leading insertion run)
    if claim.get("ties") == "ends":                       # the winning copy cut out: another end attains the distance
        assert O.hw_locate(q, t[:row[1]] + t[row[2] + 1:], -1)[0] == row[0], where
    if claim.get("ties") == "starts":                     # a larger start attains it for the same end
        assert any(O.nw_path(q, t[s:row[2] + 1])[0] == row[0] for s in range(row[1] + 1, row[2] + 1)), where


@pytest.mark.parametrize("group", E.ALL_GROUPS)
def test_every_claim_holds(group):
    rows = oracle_rows(group)
    names = [c.name for c in E.cases(group)]
    assert len(set(names)) == len(names) > 0
    for c in E.cases(group):
        assert c.group == group[0] and len(c.targets) == len(c.ks) == len(c.lanes) > 0 and c.what
        assert max(len(s) for s in [c.query] + c.targets) <= 900 and all(set(s) <= set("ACGT") and s for s in [c.query] + c.targets)
        for i in range(len(c.targets)):
            check_lane(c, i, rows[c.name, i])


def hits_of(group):
    rows = oracle_rows(group)
    return [(c, i, rows[c.name, i]) for c in E.cases(group) for i in range(len(c.targets)) if rows[c.name, i][0] >= 0]


def test_coverage_locate_and_finish_classes():
    rows = oracle_rows("a")
    for R in E.LOCATE_EDGES:
        for how in ("k", "delta"):
            c, = [c for c in E.cases("a") if c.name == "a_rows%d_by_%s" % (R, how)]
            got = [rows[c.name, i] for i in range(3)]
            assert all(restated_rows(len(t) - len(c.query), k) == R for t, k in zip(c.targets, c.ks))
            assert got[0][0] == got[1][0] == c.ks[0] and got[2] == MISS
            assert (c.ks[0] > 5) == (how == "k")
    # the locate and finish classes groups a, b and g name
    assert {E.words(restated_rows(len(t) - len(c.query), k)) for c in E.cases("a") for t, k in zip(c.targets, c.ks)} == {1, 2, 4, 8}
    assert {E.words(2 * k + 1) for c, i, r in hits_of("a") for k in [c.ks[i]]} == {1, 2, 4, 8}
    rows = oracle_rows("b")
    for k in E.FINISH_EDGES:
        c, = [c for c in E.cases("b") if c.name == "b_k%d" % k]
        got = [rows[c.name, i] for i in range(len(c.targets))]
        assert all(g[0] == k for g in got)
        assert got[0][2] - got[0][1] + 1 == len(c.query) - k                    # the end cell on diagonal -k
        assert (len(got) == 2) == (k <= 128) and (len(got) == 1 or got[1][2] - got[1][1] + 1 == len(c.query) + k)          # ... and +k
    assert {E.words(2 * k + 1) for k in E.FINISH_EDGES} == {1, 2, 4, 8}
    assert [E.words(2 * k + 1) for k in E.FINISH_CLASS_K] == [1, 2, 4, 8]


def test_coverage_blocks_ties_and_head():
    hits = hits_of("d")
    for m in E.BLOCK_TARGET_LENGTHS:
        ends = {r[2] for c, i, r in hits if c.name == "d_m%d" % m and len(c.targets[i]) == m}
        assert ends >= {e for e in E.BLOCK_ENDS if e < m} | {m - 1, 15}, m
        c, = [c for c in E.cases("d") if c.name == "d_m%d" % m]
        assert max(len(s) for s in [c.query] + c.targets) == m == c.tile["longest"]
    for P in E.BLOCK_QUERY_LENGTHS:
        mine = [(c, i, r) for c, i, r in hits if c.name == "d_P%d" % P]
        assert all(len(c.query) == P for c, i, r in mine)
        assert {r[2] for c, i, r in mine} >= {P - 3 - 1} | {e for e in E.BLOCK_ENDS if P - 1 <= e <= P + 8}, P
        assert any(r[2] == len(c.targets[i]) - 1 for c, i, r in mine)
    assert sum(c.lanes[i].get("ties") == "ends" for c, i, r in hits_of("e")) >= 3 and sum(c.lanes[i].get("ties") == "starts" for c, i, r in hits_of("e")) >= 6
    rows = oracle_rows("f")
    c = E.cases("f")[0]
    got = [rows[c.name, i] for i in range(len(c.targets))]
    assert [g[2] for g in got] == list(E.HEAD_ENDS)
    for c in E.cases("f"):                                # one tile, both branches of min(end + 1, P + kmax) among its hits
        got = [rows[c.name, i] for i in range(len(c.targets))]
        assert E.host_tiles(c) == [(c.tile["W"], list(range(len(c.targets))))] and max(c.ks) == c.tile["kmax"]
        assert any(g[2] + 1 < len(c.query) + max(c.ks) for g in got) and any(g[2] + 1 > len(c.query) + max(c.ks) for g in got)
    assert {g[2] for c in E.cases("f")[1:] for g in [rows[c.name, i] for i in range(len(c.targets))]} >= {30, 31, 32, 33, 62, 63, 64}


def test_coverage_trace_and_walk():
    hits = hits_of("g")
    for k in E.FINISH_CLASS_K:
        mine = [(c, i, r) for c, i, r in hits if c.ks[i] == k]
        assert len(mine) == len([1 for c in E.cases("g") for kk in c.ks if kk == k])          # every lane of the group is a hit
        runs = set(E.RUNS + (k,))
        assert {r[3] for c, i, r in mine if r[1] == 0} >= runs and {r[4] for c, i, r in mine} >= runs
        assert {r[4] for c, i, r in mine if r[1] == 1} >= runs                                  # the mirror: start == 1, no leading run
        assert any(r[3] > 0 and r[4] > 0 for c, i, r in mine)
        assert {r[2] - r[1] + 1 for c, i, r in mine if r[1] == 0 and r[3] >= 1} >= set(E.WINDOWS)
        assert {r[2] - r[1] + 1 for c, i, r in mine if r[1] == 1} >= set(E.WINDOWS)
        assert any(r[3] >= 1 and r[2] - r[1] + 1 > 2 * E.HW_SEG for c, i, r in mine)
        # an insertion / a deletion on the path inside the first segment and on a column that is a multiple of HW_SEG
        ops = [O.nw_path(c.query, c.targets[i][r[1]:r[2] + 1])[1] for c, i, r in mine if r[1] == 0 and r[3] >= 1]
        cols = set()
        for path in ops:
            col = 0
            for n, op in path[1:]:
                if op == "D":
                    cols.add(("D", col + 1))
                if op == "I":
                    cols.add(("I", col))
                col += n if op != "I" else 0
        assert {("D", 4), ("D", 8), ("D", 16)} <= cols and any(op == "I" and 0 < col < 8 for op, col in cols) and any(op == "I" and col % 8 == 0 and col for op, col in cols), sorted(cols)


def test_coverage_tiles_promotion_and_grid():
    rows = oracle_rows("h")
    assert sorted(len(c.targets) for c in E.cases("h") if c.tile["W"] == 1 and c.name != "h_k_spread") == sorted(E.TILE_SIZES)
    for c in E.cases("h"):
        W, n = c.tile["W"], c.tile["n"]
        got = [rows[c.name, i] for i in range(n)]
        tiles = E.host_tiles(c)
        need = [i for i in range(n) if len(c.targets[i]) - len(c.query) >= -c.ks[i]]
        assert sorted(i for w, lanes in tiles for i in lanes) == need and all(w <= W for w, lanes in tiles)
        assert all(1 <= len(lanes) <= 64 for w, lanes in tiles)
        if n >= 63:
            assert all(w == W for w, lanes in tiles) and len(tiles) == (len(need) + 63) // 64          # full tiles of the class
            assert min(c.ks) == c.tile["kmin"] and max(c.ks) == c.tile["kcap"]
            assert min(len(c.targets[i]) - len(c.query) + c.ks[i] for i in need) == 0 and max(len(t) for t in c.targets) == len(c.query) + c.tile["dmax"]
            assert sum(g[0] >= 0 for g in got) >= n // 4 and sum(g == MISS for g in got) >= n // 5 and len(need) < n
            ms0 = [g[2] - g[1] + 1 for g in got if g[0] >= 0 and g[1] == 0]
            assert min(ms0) == max(8, len(c.query) - c.tile["kcap"]) and max(ms0) >= len(c.query) - 2 and len(set(ms0)) >= 5
    c, = [c for c in E.cases("h") if c.name == "h_k_spread"]
    assert E.host_tiles(c) == [(1, list(range(len(c.targets))))] and c.ks[0] == min(c.ks) < max(c.ks) == c.ks[1]
    P, jx = len(c.query), len(c.query) - max(c.ks)
    assert rows[c.name, 1][2] + 1 == jx and (jx - 1) // 32 * 32 + 32 < P - c.ks[0]          # lane 1 ends in column jx, its block is plain by lane 0's k alone
    for c in E.cases("i"):
        W = c.tile["own_w"]
        deltas = [len(t) - len(c.query) for t in c.targets]
        assert all(E.words(restated_rows(d, k)) == W for d, k in zip(deltas, c.ks))
        assert E.words(restated_rows(max(deltas), max(c.ks))) == 2 * W == c.tile["common_w"]
        assert all(w == W for w, lanes in E.host_tiles(c)) and len(E.host_tiles(c)) >= 2
        assert all(r[0] >= 0 for r in [oracle_rows("i")[c.name, i] for i in range(len(c.targets))])
    assert sorted(c.tile["own_w"] for c in E.cases("i")) == [1, 2, 4]
    assert E.finish_grid_cap(1) == 4096 and E.finish_grid_cap(2) == 2304
    for W in (1, 2):
        cs = E.cases("j%d" % W)
        assert len(cs) == E.finish_grid_cap(W) + 200 == len({c.query for c in cs})
        cap = E.finish_grid_cap(W)
        rows = oracle_rows("j%d" % W)
        second = [(rows[cs[i].name, 0], rows[cs[i + cap].name, 0]) for i in range(200)]
        seg = lambda r: (r[2] - r[1]) // E.HW_SEG
        assert all(a[3] >= 1 and b[3] >= 1 and a[1] == b[1] == 0 for a, b in second)
        assert sum(a[3] != b[3] and a[2] != b[2] for a, b in second) >= 150 and sum(seg(a) != seg(b) for a, b in second) >= 50


# ---- the tile emulator on the designed tiles ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def run_tile(L, W, q, targets, ks):
    n = len(targets)
    arr = (ctypes.c_char_p * n)(*[t.encode() for t in targets])
    tl = (ctypes.c_int * n)(*[len(t) for t in targets])
    kk = (ctypes.c_int * n)(*ks)
    out = (ctypes.c_int32 * (5 * n))()
    L.emul_hw_tile(W, q.encode(), len(q), n, arr, tl, kk, out)
    return [list(out[5 * i:5 * i + 5]) for i in range(n)]


@pytest.mark.parametrize("group", E.ALL_GROUPS)
def test_emulator_on_the_hosts_tiles(emul, group):
    rows = oracle_rows(group)
    case_list = E.cases(group)
    if group[0] == "j":                                   # too many tiles: a slice of 64, across the grid cap
        cap = E.finish_grid_cap(int(group[1]))
        case_list = case_list[:16] + case_list[cap - 16:cap + 16] + case_list[-16:]
        assert len(case_list) == 64
    tiles = lanes = 0
    for c in case_list:
        for W, idx in E.host_tiles(c):
            got = run_tile(emul, W, c.query, [c.targets[i] for i in idx], [c.ks[i] for i in idx])
            for i, g in zip(idx, got):
                assert g == rows[c.name, i], (c.name, i, W, idx)
            tiles += 1
            lanes += len(idx)
    assert tiles >= 1 and lanes >= tiles
    if group in "fh":
        assert lanes > 2 * tiles
