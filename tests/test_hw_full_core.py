"""CPU: the lane-level math of the un-banded infix kernels (isocon_amd/csrc/hw_full_core.hpp, shared host/device header) driven
by 64 emulated lanes in lock step (tests/emul/hw_full_emul.cpp, g++) and compared with the oracle's full matrices (hw_locate +
nw_path): distance, start, end, leading and trailing insertion run -- free top row, the reversed START pass, the [step][lane]
trace store and the walk, the trailing run across blocks, the boundary buffer between passes of 64 blocks."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_hw_full_emul.so")
SRC = os.path.join(HERE, "emul", "hw_full_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_core.hpp", "hw_full_core.hpp")]


# plain and -fsanitize=undefined builds, as for the other emulators: a shift by a computed amount that is out of range is masked
# on the GPU and undefined here, so it has to be absent.
@pytest.fixture(scope="module", params=["plain", "ubsan"])
def emul(request):
    so = SO if request.param == "plain" else SO.replace(".so", "_ubsan.so")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-static-libubsan"]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRC])
    return ctypes.CDLL(so)


def run_pair(L, q, t, k):
    out = (ctypes.c_int32 * 5)()
    L.emul_hw_full_pair(q.encode(), len(q), t.encode(), len(t), k, out)
    return list(out)


def hw_row(x, y, k):
    ed, start, end = O.hw_locate(x, y, k)
    if ed < 0:
        return [-1, -1, -1, 0, 0]
    _, ops = O.nw_path(x, y[start:end + 1])
    return [ed, start, end, ops[0][0] if ops[0][1] == "I" else 0, ops[-1][0] if ops[-1][1] == "I" else 0]


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, nmut):
    v = list(s)
    for _ in range(nmut):
        p = rng.randrange(len(v)) if v else 0
        r = rng.random()
        if r < 0.4 and v:
            v[p] = rng.choice("ACGT")
        elif r < 0.7 and len(v) > 1:
            del v[p]
        else:
            v.insert(p, rng.choice("ACGT"))
    return "".join(v)


@pytest.mark.parametrize("qlen", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_pairs_equal_oracle(emul, qlen):
    rng = random.Random(qlen)
    hits = lead = trail = 0
    for mult in (1, 2, 5, 12):
        for related in (True, False):
            for k in (0, 1, qlen, 5 * qlen):
                q = rnd(rng, qlen)
                tlen = max(1, qlen * mult + rng.randint(-2, 2))
                if related:
                    # the query, a few edits and junk at its ends, somewhere inside the target (or hanging over its ends)
                    core = mutate(rng, q, rng.choice([0, 1, 3]))
                    a = rng.randint(0, max(0, tlen - len(core)))
                    t = (rnd(rng, a) + core + rnd(rng, max(0, tlen - a - len(core))))
                    if rng.random() < 0.5:
                        q = rnd(rng, rng.choice([1, 3, 9])) + q if rng.random() < 0.5 else q + rnd(rng, rng.choice([1, 3, 9]))
                    if mult == 1 and rng.random() < 0.5:
                        t = t[rng.randint(0, 3):len(t) - rng.randint(0, 3)] or "A"
                else:
                    t = rnd(rng, tlen)
                e = hw_row(q, t, k)
                assert run_pair(emul, q, t, k) == e, (q, t, k)
                hits += e[0] >= 0
                lead += e[3] > 0
                trail += e[4] > 0
    assert hits >= 8
    if qlen >= 63:
        assert lead + trail > 0


def test_negatives(emul):
    assert run_pair(emul, "ACGTACGT", "TTTTTTTTTTTT", 2) == [-1, -1, -1, 0, 0]          # distance above k
    assert run_pair(emul, "ACGTACGTACGT", "ACG", 3) == [-1, -1, -1, 0, 0]               # query longer than target + k
    assert run_pair(emul, "ACGTACGTACGT", "ACG", 9) == hw_row("ACGTACGTACGT", "ACG", 9)
    assert run_pair(emul, "", "ACG", 3) == [-1, -1, -1, 0, 0]


def test_trailing_run_crosses_blocks(emul):
    rng = random.Random(11)
    core = rnd(rng, 60)
    for junk in (5, 70, 140):
        q = core + "A" * junk                # the target ends where the core does: the query's tail is one insertion run
        t = rnd(rng, 30).replace("A", "C") + core
        e = hw_row(q, t, junk + 5)
        assert e[4] >= junk and run_pair(emul, q, t, junk + 5) == e
        q2 = "A" * junk + core               # and a leading run at start == 0
        t2 = core + rnd(rng, 30).replace("A", "C")
        e2 = hw_row(q2, t2, junk + 5)
        assert e2[3] >= junk and e2[1] == 0 and run_pair(emul, q2, t2, junk + 5) == e2


@pytest.mark.parametrize("qlen", [4097, 4200])
def test_second_pass_of_the_block_loop(emul, qlen):
    """Queries above 4 096 rows: the boundary row's deltas go through the 2-bit buffer, the trace store has two passes."""
    rng = random.Random(qlen)
    core = rnd(rng, qlen - 40)
    q = rnd(rng, 25) + core + rnd(rng, 15)
    for t in (mutate(rng, core, 6) + rnd(rng, 150), rnd(rng, 200) + mutate(rng, core, 6)):
        e = hw_row(q, t, 600)
        assert e[0] >= 0 and run_pair(emul, q, t, 600) == e


def test_trace_layout(emul):
    for m, ms in [(1, 1), (64, 3), (65, 100), (700, 513), (4096, 70), (4097, 70), (8300, 33)]:
        assert emul.emul_hw_full_layout_ok(m, ms) == 1
