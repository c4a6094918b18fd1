"""CPU: the lane-level math of the global alignment path kernels (isocon_amd/csrc/nw_path_core.hpp on top of hw_full_core.hpp, shared
host/device headers) driven by 64 emulated lanes in lock step (tests/emul/nw_path_emul.cpp, g++) and compared with the oracle's full
matrix (nw_path): the distance and the whole op list -- the TRACE pass over the whole target, the walk with its border continuation,
the '=' / 'X' decision from the two bases, the reversed runs and the forward list, the boundary buffer between passes of 64 blocks.
The sanitizer build (-fsanitize=undefined,address) is a stand-alone program run as a subprocess over the same cases."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_nw_path_emul.so")
EXE = os.path.join(HERE, "emul", "_nw_path_emul_san")
SRC = os.path.join(HERE, "emul", "nw_path_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_core.hpp", "hw_full_core.hpp", "nw_path_core.hpp")]
QLENS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [SRC] + CORES)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.emul_forward_runs.restype = ctypes.c_int64
    return L


def run_pair(L, q, t):
    ops = np.zeros(len(q) + len(t) + 2, dtype=np.uint32)
    n_ops, n_rev = ctypes.c_int64(0), ctypes.c_int64(0)
    ed = L.emul_nw_path(q.encode(), len(q), t.encode(), len(t), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(n_ops), ctypes.byref(n_rev))
    return ed, [(int(o >> 4), "=XID"[int(o & 15)]) for o in ops[:n_ops.value]], n_rev.value


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, nmut, ends=False):
    v = list(s)
    for e in range(nmut):
        p = rng.randrange(len(v)) if v else 0
        if ends and e < 2:
            p = 0 if e == 0 else max(len(v) - 1, 0)          # an edit at either end
        r = rng.random()
        if r < 0.4 and v:
            v[p] = rng.choice("ACGT")
        elif r < 0.7 and len(v) > 1:
            del v[p]
        else:
            v.insert(p + (1 if ends and e == 1 else 0), rng.choice("ACGT"))
    return "".join(v)


def length_cases(qlen):
    """related targets with 0-6 edits (some at either end), and unrelated ones"""
    rng = random.Random(1000 + qlen)
    out = []
    for nmut in range(7):
        q = rnd(rng, qlen)
        out.append((q, mutate(rng, q, nmut, ends=nmut >= 2 and nmut % 2 == 0)))
    for tlen in (1, max(1, qlen - 1), qlen, qlen + 3, 2 * qlen + 1):
        out.append((rnd(rng, qlen), rnd(rng, tlen)))
    return out


def border_cases():
    """paths that end -- at the walk's end, i.e. begin -- in a run of I or of D longer than 64 (the border continuation crosses blocks),
    and such runs at the path's end"""
    rng = random.Random(11)
    core = rnd(rng, 60)
    out = []
    for junk in (5, 70, 140):
        out += [("A" * junk + core, core.replace("A", "C")), (core.replace("A", "C"), "A" * junk + core),
                (core + "A" * junk, core.replace("A", "C")), (core.replace("A", "C"), core + "A" * junk)]
    return out


def long_cases():
    """one 4 097-row query against a related target and one against a 150-base target: two passes, the boundary buffer, hundreds of runs"""
    rng = random.Random(4097)
    q = rnd(rng, 4097)
    return [(q, mutate(rng, q, 6, ends=True)), (q, rnd(rng, 150))]


ALL_CASES = [c for n in QLENS for c in length_cases(n)] + border_cases() + long_cases() + [("", "ACG"), ("ACG", ""), ("", "")]
_EXPECT = {}


def expect(q, t):
    """the oracle's answer, computed once per pair and shared by the tests"""
    if (q, t) not in _EXPECT:
        _EXPECT[(q, t)] = O.nw_path(q, t)
    return _EXPECT[(q, t)]


@pytest.mark.parametrize("qlen", QLENS)
def test_paths_equal_oracle(emul, qlen):
    edits = 0
    for q, t in length_cases(qlen):
        ed, ops = expect(q, t)
        got_ed, got_ops, n_rev = run_pair(emul, q, t)
        assert (got_ed, got_ops) == (ed, ops), (q, t)
        assert n_rev == len(ops) <= 2 * ed + 1          # the walk emits maximal runs, and the bound the op storage is sized from
        edits += ed > 0
    assert edits >= 6


def test_border_runs_cross_blocks(emul):
    seen = set()
    for q, t in border_cases():
        ed, ops = expect(q, t)
        assert run_pair(emul, q, t)[:2] == (ed, ops), (q, t)
        for where in (0, -1):
            if ops[where][1] in "ID" and ops[where][0] > 64:
                seen.add((where, ops[where][1]))
    assert seen == {(0, "I"), (0, "D"), (-1, "I"), (-1, "D")}


def test_second_pass_of_the_block_loop(emul):
    (q, related), (_, short) = long_cases()
    ed, ops = expect(q, related)
    assert 0 < ed <= 6 and run_pair(emul, q, related)[:2] == (ed, ops)
    ed, ops = expect(q, short)
    assert len(ops) >= 200 and run_pair(emul, q, short)[:2] == (ed, ops)


def test_empty_sequences(emul):
    assert run_pair(emul, "", "ACG")[:2] == (3, [(3, "D")]) == expect("", "ACG")
    assert run_pair(emul, "ACG", "")[:2] == (3, [(3, "I")]) == expect("ACG", "")
    assert run_pair(emul, "", "")[:2] == (0, [])


def test_forward_runs_helper(emul):
    def fwd(rev):
        a = np.array([(n << 4) | c for n, c in rev], dtype=np.uint32)
        out = np.zeros(max(len(a), 1), dtype=np.uint32)
        p = ctypes.POINTER(ctypes.c_uint32)
        n = emul.emul_forward_runs(a.ctypes.data_as(p), len(a), out.ctypes.data_as(p))
        assert n == emul.emul_forward_runs(a.ctypes.data_as(p), len(a), None)          # count only
        return [(int(o >> 4), int(o & 15)) for o in out[:n]]
    assert fwd([(7, 0)]) == [(7, 0)]                                                     # a single op
    assert fwd([(2, 2), (3, 2), (1, 0), (4, 1)]) == [(4, 1), (1, 0), (5, 2)]              # equal neighbours merge
    assert fwd([(2, 2), (0, 0), (3, 2), (4, 1), (4, 1)]) == [(8, 1), (5, 2)]              # also across an empty run
    assert fwd([]) == []


def test_sanitizer_program():
    """-fsanitize=undefined,address on a stand-alone program (its own main) over the same cases, as a subprocess"""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DNWP_EMUL_MAIN", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-o", EXE, SRC])
    text = "".join("%s %s\n" % (q or "-", t or "-") for q, t in ALL_CASES)
    r = subprocess.run([EXE], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(ALL_CASES)
    for (q, t), ln in zip(ALL_CASES, lines):
        f = [int(x) for x in ln.split()]
        ed, ops = expect(q, t)
        assert (f[0], [(o >> 4, "=XID"[o & 15]) for o in f[1:]]) == (ed, ops), (q, t)
