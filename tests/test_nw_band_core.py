"""CPU: the lane-level math of the banded global alignment path kernels (isocon_amd/csrc/nw_band_core.hpp, a shared host/device header)
driven by one emulated lane (tests/emul/nw_band_emul.cpp, g++) and compared with the oracle's full matrix (nw_path / hw_path): the class
from the known distance, the window origin, the forward pass through the sliding window, the score on the final diagonal, and the walk
that does not take a step out of the window -- distance and the whole op list.  The sanitizer build (-fsanitize=undefined,address) is a
stand-alone program run as a subprocess over the same cases."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_nw_path_core import ALL_CASES, rnd

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_nw_band_emul.so")
EXE = os.path.join(HERE, "emul", "_nw_band_emul_san")
SRC = os.path.join(HERE, "emul", "nw_band_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f)
         for f in ("band_core.hpp", "ed_lanes_core.hpp", "hw_core.hpp", "hw_full_core.hpp", "nw_path_core.hpp", "nw_band_core.hpp")]
EDGE_LENGTHS = [63, 64, 127, 128, 255, 256]
NOT_BANDED = 0
_EXPECT = {}


def expect(q, t):
    """the oracle's answer, computed once per pair and shared by the tests"""
    if (q, t) not in _EXPECT:
        _EXPECT[(q, t)] = O.nw_path(q, t)
    return _EXPECT[(q, t)]


def corridor(m, n, ed):
    """the diagonals an optimal path of distance ed can touch: |d| + 2 ((ed - |d|) // 2) + 1"""
    ad = abs(m - n)
    return ad + 2 * ((ed - ad) // 2) + 1


def band_class(m, n, ed):
    """the smallest W of 1, 2, 4 whose 64 W diagonals hold the corridor, NOT_BANDED beyond 256 diagonals (and for an empty sequence,
    which the host answers)"""
    if m == 0 or n == 0:
        return NOT_BANDED
    c = corridor(m, n, ed)
    return 1 if c <= 64 else 2 if c <= 128 else 4 if c <= 256 else NOT_BANDED


def banded_path_cases():
    """(a): the cases of the un-banded kernels' test whose corridor is at most 256 diagonals"""
    return [(q, t) for q, t in ALL_CASES if q and t and band_class(len(q), len(t), expect(q, t)[0])]


def tie_cases():
    """(b): homopolymers and dinucleotide repeats of unequal length -- every cell of the corridor is a tie"""
    out = [("A" * 50, "A" * 45), ("A" * 45, "A" * 50), ("AC" * 40, "CA" * 38), ("CA" * 38, "AC" * 40), ("A" * 30, "A" * 30), ("AC" * 20, "A" * 33),
           ("A" * 70, "A" * 3), ("A", "A" * 64), ("AC" * 60, "AC" * 20 + "CA" * 37), ("ACG" * 30, "AGC" * 28)]
    return out


def sweep_cases():
    """(b): random pairs over the alphabets A, AC and ACGT, up to 40 bases, 0-8 edits or unrelated"""
    rng = random.Random(404)
    out = []
    for alphabet in ("A", "AC", "ACGT"):
        for _ in range(400):
            q = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 40)))
            if rng.random() < 0.3:
                t = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 40)))
            else:
                v = list(q)
                for _ in range(rng.randint(0, 8)):
                    r, p = rng.random(), rng.randrange(len(v) + 1)
                    if r < 0.4 and p < len(v):
                        v[p] = rng.choice(alphabet)
                    elif r < 0.7 and len(v) > 1 and p < len(v):
                        del v[p]
                    else:
                        v.insert(p, rng.choice(alphabet))
                t = "".join(v)[:40]
            out.append((q, t))
    return out


def edge_cases():
    """(c): a block of L random bases inserted into a random 600-base sequence, at the start, in the middle and at the end, on the query
    side and on the target side: ed = L exactly and the corridor is L + 1 diagonals.  [(L, q, t)]"""
    rng = random.Random(600)
    out = []
    for L in EDGE_LENGTHS:
        for where in (0, 300, 600):
            s, block = rnd(rng, 600), rnd(rng, L)
            longer = s[:where] + block + s[where:]
            out += [(L, longer, s), (L, s, longer)]
    return out


def window_cases():
    """(d): a query inside a target with flanks of 37 and 20 bases: (q, t); the window comes from the oracle's location.  Every class
    edge of (c), the block on either side: with the block in the query the located window's path holds it whole (distance L); with the
    block in the target an infix alignment skips a block at either end and pays L for one in the middle -- the class is taken from the
    oracle's distance and window either way, and the blocks of 256 bases are not banded"""
    rng = random.Random(37)
    out = []
    for L, q, t in edge_cases():
        out.append((q, rnd(rng, 37) + t + rnd(rng, 20)))
    # (of the blocks of 256 bases only the one in the query's middle keeps its distance in infix form -- a block at an end aligns partly
    # with the flank, and 300 query bases against a random block cost less than deleting it: two more blocks beyond the band, of 300
    # bases in the query's middle, at the head of the list and inside it, so that un-banded hits and band hits alternate)
    for at in (0, 20):
        s, block = rnd(rng, 600), rnd(rng, 300)
        out.insert(at, (s[:300] + block + s[300:], rnd(rng, 37) + s + rnd(rng, 20)))
    for n in (30, 65, 200):
        for nmut in (0, 3, 7):
            q = rnd(rng, n)
            v = list(q)
            for _ in range(nmut):
                p = rng.randrange(len(v))
                if rng.random() < 0.5:
                    v[p] = rng.choice("ACGT")
                elif rng.random() < 0.5 and len(v) > 1:
                    del v[p]
                else:
                    v.insert(p, rng.choice("ACGT"))
            out.append((q, rnd(rng, 37) + "".join(v) + rnd(rng, 20)))
    return out


def expect_window(q, t):
    """(ed, start, cols, ops) of the oracle's infix path"""
    key = ("hw", q, t)
    if key not in _EXPECT:
        e = O.hw_path(q, t, -1)
        (start, end), = e["locations"]
        _EXPECT[key] = (e["editDistance"], start, end - start + 1, expect(q, t[start:end + 1])[1])
    return _EXPECT[key]


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [SRC] + CORES)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def run_pair(L, q, t, ed, start=0, cols=None, last=False):
    """(class, score or status, ops, reversed runs)"""
    cols = len(t) - start if cols is None else cols
    ops = np.zeros(len(q) + len(t) + 2, dtype=np.uint32)
    n_ops, n_rev, cls = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(-1)
    sc = L.emul_nw_band(q.encode(), len(q), t.encode(), len(t), start, cols, ed, int(last), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                        ctypes.byref(n_ops), ctypes.byref(n_rev), ctypes.byref(cls))
    return cls.value, sc, [(int(o >> 4), "=XID"[int(o & 15)]) for o in ops[:n_ops.value]], n_rev.value


def check(L, q, t, last=False):
    ed, ops = expect(q, t)
    cls, sc, got, n_rev = run_pair(L, q, t, ed, last=last)
    assert cls == band_class(len(q), len(t), ed), (q, t)
    if cls != NOT_BANDED:
        assert (sc, got) == (ed, ops), (q, t, last)
        assert n_rev == len(ops) <= 2 * ed + 1
    return cls


def test_class_of_a_pair(emul):
    assert [emul.emul_nwb_class(d, ed) for d, ed in ((0, 0), (0, 63), (0, 64), (0, 65), (5, 4), (-63, 63), (64, 64), (-127, 128), (128, 128), (0, 255), (0, 257), (256, 256))] == \
        [1, 1, 2, 2, 0, 1, 2, 2, 4, 4, 0, 0]
    for d in range(-300, 301, 7):
        for ed in range(abs(d), 300, 3):
            assert emul.emul_nwb_class(d, ed) == band_class(600 + d, 600, ed)


def test_paths_of_the_unbanded_cases(emul):
    cases = banded_path_cases()
    assert len(cases) >= 100
    seen = {check(emul, q, t) for q, t in cases}
    assert {1, 2} <= seen
    assert all(check(emul, q, t, last=True) for q, t in cases)
    dropped = [(q, t) for q, t in ALL_CASES if q and t and (q, t) not in set(cases)]
    assert dropped and all(check(emul, q, t) == NOT_BANDED for q, t in dropped)


@pytest.mark.parametrize("last", [False, True], ids=["corridor_on_first_diagonal", "corridor_on_last_diagonal"])
def test_tie_heavy_pairs(emul, last):
    for q, t in tie_cases() + sweep_cases():
        assert check(emul, q, t, last=last) != NOT_BANDED


def test_class_edges(emul):
    seen = []
    for L, q, t in edge_cases():
        ed, _ = expect(q, t)
        assert ed == L and corridor(len(q), len(t), ed) == L + 1
        cls = check(emul, q, t)
        assert cls == {63: 1, 64: 2, 127: 2, 128: 4, 255: 4, 256: NOT_BANDED}[L]
        if cls:
            assert check(emul, q, t, last=True) == cls
        seen.append(cls)
    assert len(seen) == 36


def test_window_form(emul):
    classes, unaligned, at_edge = {1: 0, 2: 0, 4: 0, NOT_BANDED: 0}, 0, set()
    for q, t in window_cases():
        ed, start, cols, ops = expect_window(q, t)
        for last in (False, True):
            cls, sc, got, _ = run_pair(emul, q, t, ed, start, cols, last)
            assert cls == band_class(len(q), cols, ed), (q, t, start, cols)
            if cls != NOT_BANDED:
                assert (sc, got) == (ed, ops), (q, t, start, cols, last)
        classes[cls] += 1
        unaligned += start % 32 != 0
        if corridor(len(q), cols, ed) in (64, 65, 128, 129, 256, 257):
            at_edge.add(corridor(len(q), cols, ed))
    # every class edge is met in window form, from both sides; three blocks in the query's middle are not banded
    assert at_edge == {64, 65, 128, 129, 256, 257}
    assert classes[1] >= 10 and classes[2] >= 6 and classes[4] >= 6 and classes[NOT_BANDED] == 3 and unaligned >= 30
    q, t = window_cases()[0]
    assert run_pair(emul, q, t, 3, 40, len(t))[1] == -7 and run_pair(emul, q, t, 3, -1, 5)[1] == -7          # a window outside the target


def test_wrong_distance_is_noticed(emul):
    """the pass' score is compared with the known distance: a claimed distance that is not the pair's gives no path"""
    q = "ACGTACGTAC" * 6
    t = q[:20] + q[26:]
    ed, ops = expect(q, t)
    assert ed == 6 and run_pair(emul, q, t, ed)[1:3] == (ed, ops)
    cls, sc, got, _ = run_pair(emul, q, t, ed + 4)
    assert (cls, sc, got) == (1, ed, [])          # the score is the true distance, not the claimed one: no walk


def test_sanitizer_program():
    """-fsanitize=undefined,address on a stand-alone program (its own main) over the same cases, as a subprocess"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DNWB_EMUL_MAIN", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-o", EXE, SRC])
    cases = []          # (q, t, start, cols, ed, last, ops)
    for q, t in banded_path_cases() + tie_cases() + sweep_cases() + [(q, t) for _, q, t in edge_cases()]:
        ed, ops = expect(q, t)
        for last in (0, 1):
            cases.append((q, t, 0, len(t), ed, last, ops))
    for q, t in window_cases():
        ed, start, cols, ops = expect_window(q, t)
        for last in (0, 1):
            cases.append((q, t, start, cols, ed, last, ops))
    text = "".join("%s %s %d %d %d %d\n" % c[:6] for c in cases)
    r = subprocess.run([EXE], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (q, t, start, cols, ed, last, ops), ln in zip(cases, lines):
        f = [int(x) for x in ln.split()]
        assert f[0] == band_class(len(q), cols, ed)
        if f[0]:
            assert (f[1], [(o >> 4, "=XID"[o & 15]) for o in f[2:]]) == (ed, ops), (q, t, start, cols, last)
