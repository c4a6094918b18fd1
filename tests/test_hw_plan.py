"""CPU: what the host decides for the banded infix kernels without a device (isocon_amd/csrc/hw_plan.hpp: the greedy cut of a pair list into
tiles with its LOCATE-shaped and FINISH-shaped rules, the grid of the finish stage, the window words of a band) against the restatements of
tests/hw_edge_cases.py -- tests/emul/hw_plan_emul.cpp, a program of its own, built with g++ and a second time with
-fsanitize=address,undefined.  The program itself checks every cut: each pair that needs a kernel in exactly one lane, 64 lanes per tile with
the empty ones at its tail, one query per tile, the common window of a tile within its class."""
import os
import subprocess

import pytest

import hw_edge_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "hw_plan_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("hw_plan.hpp", "hw_core.hpp", "band_core.hpp")]
CLASSES = (1, 2, 4, 8)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def ask(request):
    """ask(text) -> the program's answer to the commands of `text`, as lines"""
    exe = os.path.join(HERE, "emul", "_hw_plan_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])

    def run(text):
        done = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert done.returncode == 0, (done.stdout[-1000:] + done.stderr)[-3000:]
        return done.stdout.splitlines()
    return run


def tiles_of(lines):
    """[[(W, query, [pairs]), ...] per cut] of the answers to locate / finish commands"""
    cuts, cur = [], []
    for ln in lines:
        if ln == "end":
            cuts.append(cur)
            cur = []
        else:
            f = ln.split()
            assert f[0] == "tile"
            cur.append((int(f[1]), int(f[2]), [int(x) for x in f[3:]]))
    assert not cur
    return cuts


def locate_command(lens, q, t, k):
    return "locate %d %d\n%s\n%s\n" % (len(lens), len(q), " ".join(map(str, lens)), "\n".join("%d %d %d" % x for x in zip(q, t, k)))


def test_locate_cut_against_the_restated_rule(ask):
    """every case of groups h (tiles of 1, 2, 63, 64, 65, 130 lanes) and i (pairs of W words whose common window needs 2 W), one store per
    case: the query is sequence 0, target i is sequence 1 + i and pair i"""
    case_list = [c for g in "hi" for c in E.cases(g)]
    assert {c.tile["n"] for c in E.cases("h")} >= set(E.TILE_SIZES) and {c.tile["own_w"] for c in E.cases("i")} == set(E.PROMOTIONS)
    text = "".join(locate_command([len(c.query)] + [len(x) for x in c.targets], [0] * len(c.ks), range(1, 1 + len(c.ks)), c.ks) for c in case_list)
    cuts = tiles_of(ask(text))
    assert len(cuts) == len(case_list)
    for c, got in zip(case_list, cuts):
        exp = E.host_tiles(c)
        assert [(W, lanes) for W, _, lanes in got] == exp and all(query == 0 for _, query, _ in got), c.name
        assert [sum(1 for t in got if t[0] == W) for W in CLASSES] == [sum(1 for t in exp if t[0] == W) for W in CLASSES], c.name
    # the promotions are separated: no tile of an i case holds both kinds
    for c, got in zip(case_list, cuts):
        if c.group == "i":
            assert all(W == c.tile["own_w"] and len({i % 2 for i in lanes}) == 1 for W, _, lanes in got) and len(got) >= 2, c.name


def test_locate_cut_of_the_fall_back_list(ask):
    """the 2048 pairs of test_gpu_hw_edges.test_fall_back_from_device_tiles_to_host_tiles: one query, two targets in turn that fit 512
    diagonals each and not together"""
    lens, q, t, k = [300, 680, 295], [0] * 2048, [1, 2] * 1024, [20, 200] * 1024
    assert E.words(E.rows(380, 20)) == E.words(E.rows(-5, 200)) == 8 and E.words(E.rows(380, 200)) == 0
    as_case = E.Case("fall_back", "-", "A" * lens[0], ["A" * lens[x] for x in t], k, "", [], {})
    exp = E.host_tiles(as_case)
    (got,) = tiles_of(ask(locate_command(lens, q, t, k)))
    assert [(W, lanes) for W, _, lanes in got] == exp
    assert 2 * 1024 // 64 < len(got) <= 2048 and all(W == 8 for W, _, _ in got)


def test_finish_cut(ask):
    text, sizes = "", (1, 64, 65)
    for kk in E.FINISH_CLASS_K:
        for n in sizes:
            text += "finish 3 %d\n%s\n" % (n, "\n".join("2 %d" % kk for _ in range(n)))
    mixed = [31, 32] * 40
    text += "finish 1 %d\n%s\n" % (len(mixed), "\n".join("0 %d" % kk for kk in mixed))
    cuts = tiles_of(ask(text))
    assert len(cuts) == len(E.FINISH_CLASS_K) * len(sizes) + 1
    for i, kk in enumerate(E.FINISH_CLASS_K):
        assert E.words(2 * kk + 1) == CLASSES[i]
        for j, n in enumerate(sizes):
            got = cuts[i * len(sizes) + j]
            # thresholds 20, 50, 100, 200 -> classes 1, 2, 4, 8; 1, 64, 65 hits of one query -> 1, 1, 2 tiles, filled in list order
            assert [W for W, _, _ in got] == [CLASSES[i]] * (1, 1, 2)[j] and all(query == 2 for _, query, _ in got)
            assert [p for _, _, lanes in got for p in lanes] == list(range(n)) and len(got[0][2]) == min(n, 64)
    # 2 x 31 + 1 = 63 and 2 x 32 + 1 = 65 diagonals of one query: a tile of each class
    assert cuts[-1] == [(1, 0, list(range(0, 80, 2))), (2, 0, list(range(1, 80, 2)))]


def store_bytes(W, cols):
    """the column store of one workgroup of k_hw_finish<W> (csrc/hw.hpp: checkpoints every HW_SEG-th column for W <= 2, else every column;
    2 W x 64 words of 8 bytes each)"""
    return (cols // E.HW_SEG + 2 if W <= 2 else cols + 1) * 2 * W * 64 * 8


def test_finish_grid(ask):
    GiB = 1 << 30
    caps = [ln.split() for ln in ask("".join("cap %d\n" % W for W in CLASSES))]
    assert [int(c[0]) for c in caps] == [E.finish_grid_cap(W) for W in CLASSES] and [int(c[0]) for c in caps[:2]] == [4096, 2304]
    assert [int(c[1]) for c in caps] == [0, E.HW_SEG * 2 * 2 * 64 * 8, 0, 0]
    shapes = [(W, cols) for W in CLASSES for cols in (1, 7, 8, 100, 1001, 20000)]
    assert [int(x) for x in ask("".join("store %d %d\n" % s for s in shapes))] == [store_bytes(*s) for s in shapes]
    asked, exp = [], []
    for W in CLASSES:
        cap, small, large = E.finish_grid_cap(W), store_bytes(W, 100), store_bytes(W, 100000)
        assert (cap + 200) * small < 12 * GiB < cap * large
        asked += [(10, W, 100, 1 << 62), (cap, W, 100, 1 << 62), (cap + 200, W, 100, 1 << 62)]          # the tiles, then the cap
        exp += [10, cap, cap]
        asked += [(100, W, 100, 3 * (3 * small + small // 2)), (cap + 200, W, 100000, 3 * (3 * large + large // 2))]          # a third of what is free
        exp += [3, 3]
        asked += [(cap + 200, W, 100000, 1 << 62)]          # 12 GiB
        exp += [12 * GiB // large]
        asked += [(100, W, 100, 3 * small - 1), (100, W, 100, 0), (0, W, 100, 1 << 62)]          # one store exceeds the budget; never 0
        exp += [1, 1, 1]
    assert [int(x) for x in ask("".join("grid %d %d %d %d\n" % a for a in asked))] == exp


def test_band_words(ask):
    edges = [r for w in (64, 128, 256, 512) for r in (w, w + 1)]
    got = [tuple(int(x) for x in ln.split()) for ln in ask("".join("words %d\n" % r for r in [1] + edges))]
    assert [w for w, _ in got] == [1, 1, 2, 2, 4, 4, 8, 8, 0] == [E.words(r) for r in [1] + edges]
    assert [c for w, c in got if w] == [0, 0, 1, 1, 2, 2, 3, 3]
