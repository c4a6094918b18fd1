"""CPU: the index arithmetic of the device-built candidate graph (isocon_amd/csrc/hw_graph_core.hpp) compiled with g++ into a program of
its own (tests/emul/hw_graph_core_main.cpp), a second time with -fsanitize=undefined,address: per-entry counts, the slot -> (query,
neighbour) map and the reverse-slot map against end_invariant_functions._window_pairs, the end rules against _ends_adjusted."""
import os
import random
import subprocess

import numpy as np
import pytest

from isocon_amd import end_invariant_functions as END

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "hw_graph_core_main.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_graph_core.hpp")]
DEPTHS = [0, 1, 2, 5, None, 2 ** 32]          # None: n


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request):
    exe = os.path.join(HERE, "emul", "_hw_graph_core" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def check_list(exe, lens, window, depth):
    n = len(lens)
    done = subprocess.run([exe, "pairs", str(window), str(depth), str(n)] + [str(v) for v in lens], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.splitlines()
    q, t = END._window_pairs(np.asarray(lens, dtype=np.int64), 0, n, window, depth)
    assert int(lines[0]) == len(q)
    got_q, got_t, rev, own, counts = [], [], [], [], {}
    for ln in lines[1:]:
        f = [int(x) for x in ln.split()]
        if len(f) == 3:
            counts[f[0]] = (f[1], f[2])
        else:
            got_q.append(f[0]); got_t.append(f[2]); rev.append(f[3]); own.append(f[1:2] + f[4:5])
    assert got_q == q.tolist() and got_t == t.tolist()
    assert sorted(counts) == list(range(n))
    first = [0]
    for i in range(n):
        cd, cu = counts[i]
        assert cd == sum(1 for a, b in zip(got_q, got_t) if a == i and b < i) and cu == sum(1 for a, b in zip(got_q, got_t) if a == i and b > i)
        first.append(first[-1] + cd + cu)
    for p, (i, nb, rr, (r, r_own)) in enumerate(zip(got_q, got_t, rev, own)):
        assert r == r_own == p - first[i]                           # the slot of a neighbour found again from the neighbour
        assert rr < first[nb + 1] - first[nb]
        assert got_q[first[nb] + rr] == nb and got_t[first[nb] + rr] == i          # the reverse slot holds the pair the other way round
    return len(q)


def lists(window):
    rng = random.Random(window)
    w = window
    yield "empty", []
    yield "one", [100]
    yield "two_near", [100, 100 + w]
    yield "two_far", [100, 101 + w]
    yield "equal", [250] * 9
    yield "gaps_window", [100 + w * i for i in range(8)]
    yield "gaps_window_plus_1", [100 + (w + 1) * i for i in range(8)]
    yield "gaps_mixed", list(np.cumsum([100] + [w if i % 2 else w + 1 for i in range(9)]))
    # runs of equal lengths exactly at, and one beyond, either edge of the middle run's window
    yield "runs_at_edges", [200 - w] * 3 + [200] * 4 + [200 + w] * 3
    yield "runs_past_edges", [199 - w] * 3 + [200 - w] * 2 + [200] * 4 + [200 + w] * 2 + [201 + w] * 3
    yield "random", sorted(rng.randint(100, 100 + 6 * max(w, 1)) for _ in range(40))
    yield "random_dense", sorted(rng.randint(100, 100 + max(w, 1)) for _ in range(30))


@pytest.mark.parametrize("window", [0, 1, 10, 40])
def test_slots_and_reverse_slots_equal_window_pairs(prog, window):
    pairs = 0
    for name, lens in lists(window):
        for depth in DEPTHS:
            pairs += check_list(prog, [int(v) for v in lens], window, len(lens) if depth is None else depth)
    assert pairs > 1000


def test_end_rules_equal_ends_adjusted(prog):
    rng = random.Random(5)
    for T, max_ed in [(0, 10), (5, 10), (15, 10), (121, 10), (15, 3)]:
        rows, len_t = [], []
        for _ in range(400):
            lt = rng.randint(1, 400)
            if rng.random() < 0.2:
                rows.append([-1, -1, -1, 0, 0])
            else:
                start = rng.randint(0, lt - 1)
                end = rng.randint(start, lt - 1)
                rows.append([rng.randint(0, 14), start if rng.random() < 0.7 else rng.randint(0, min(lt - 1, T + 3)),
                             end if rng.random() < 0.3 else lt - 1 - rng.randint(0, min(lt - 1, T + 3)), rng.randint(0, 2 * T + 2) * (rng.random() < 0.5),
                             rng.randint(0, 2 * T + 2) * (rng.random() < 0.5)])
            len_t.append(lt)
        text = "".join("%d %d %d %d %d %d\n" % (tuple(r) + (lt,)) for r, lt in zip(rows, len_t))
        done = subprocess.run([prog, "adjust", str(T), str(max_ed), str(len(rows))], input=text, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]
        got = [int(x) for x in done.stdout.split()]
        adj = END._ends_adjusted(np.asarray(rows), len_t, T)
        expect = [int(v) if r[0] >= 0 and 0 <= v <= max_ed else -1 for v, r in zip(adj, rows)]
        assert got == expect
        assert sum(v >= 0 for v in expect) >= 10 and sum(v < 0 for v in expect) >= 10          # (both outcomes occur in the inputs)
