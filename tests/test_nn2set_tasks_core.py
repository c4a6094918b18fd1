"""CPU: how the depth-limited 2-set search cuts a read's listed pairs into the tasks of its block test (nn2_cut_list / nn2_cut_tasks,
isocon_amd/csrc/nn2_depth_core.hpp, the shared host/device header) driven through tests/emul/nn2_tasks_main.cpp: a program of its own,
built with g++ and a second time with -fsanitize=undefined.  Every tested pair lies in exactly one task, no task holds more than 64
pairs or pairs of two reads, a task's pairs are consecutive in the list's order, and a read without a tested pair makes no task."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "nn2_tasks_main.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "nn2_depth_core.hpp")]
TASK = 64


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def exe(request):
    path = os.path.join(HERE, "emul", "_nn2_tasks" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", path, SRC])
    return path


def cut(exe, pairs):
    """pairs: [(read, tested)] -> [(read, first, count)] in the order the routine emitted them"""
    text = "%d\n" % len(pairs) + "".join("%d %d\n" % (r, int(t)) for r, t in pairs)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    out = [line for line in out if line]
    assert out[-1].startswith("tasks ")
    tasks = [tuple(int(v) for v in line.split()) for line in out[:-1]]
    assert int(out[-1].split()[1]) == len(tasks)
    return tasks


def check(exe, pairs):
    tasks = cut(exe, pairs)
    covered = [0] * len(pairs)
    for read, first, count in tasks:
        assert 1 <= count <= TASK
        assert first + count <= len(pairs)
        assert all(pairs[p][0] == read for p in range(first, first + count)), "a task spans two reads"
        assert pairs[first][1] and pairs[first + count - 1][1], "a task starts and ends with a tested pair"
        for p in range(first, first + count):          # (consecutive slots: the order inside a task is the list's)
            covered[p] += 1
    for p, (read, tested) in enumerate(pairs):
        assert covered[p] <= 1
        if tested:
            assert covered[p] == 1, "tested pair %d is in no task" % p
    # tasks of a run follow each other in the list's order
    assert [t[1] for t in tasks] == sorted(t[1] for t in tasks)
    return tasks


RUNS = [0, 1, 63, 64, 65, 128, 129]


def test_empty_list(exe):
    assert check(exe, []) == []


@pytest.mark.parametrize("n", RUNS)
def test_one_run_all_tested(exe, n):
    tasks = check(exe, [(7, 1)] * n)
    assert [t[2] for t in tasks] == [TASK] * (n // TASK) + ([n % TASK] if n % TASK else [])
    assert [t[1] for t in tasks] == list(range(0, n, TASK))


@pytest.mark.parametrize("n", RUNS[1:])
def test_untested_pairs_at_the_ends_and_in_the_middle(exe, n):
    for where in ("front", "back", "both", "middle"):
        flags = [1] * n
        if where in ("front", "both"):
            flags[0] = 0
        if where in ("back", "both"):
            flags[-1] = 0
        if where == "middle":
            for p in range(n // 3, n // 3 + max(1, n // 4)):
                flags[p] = 0
        tasks = check(exe, [(3, f) for f in flags])
        if not any(flags):
            assert tasks == []
        else:
            # the first task starts at the first tested pair and nothing reaches behind the last one
            assert tasks[0][1] == flags.index(1)
            assert tasks[-1][1] + tasks[-1][2] == n - flags[::-1].index(1)
            # never more tasks than whole groups of 64 need
            assert len(tasks) <= (n + TASK - 1) // TASK


def test_a_read_without_a_tested_pair_makes_no_task(exe):
    pairs = [(1, 1)] * 3 + [(2, 0)] * 70 + [(5, 1)] * 2 + [(6, 0)] + [(9, 1)]
    tasks = check(exe, pairs)
    assert [t[0] for t in tasks] == [1, 5, 9]
    assert tasks == [(1, 0, 3), (5, 73, 2), (9, 76, 1)]
    assert check(exe, [(4, 0)] * 129) == []


def test_runs_of_every_size_side_by_side(exe):
    pairs = []
    for read, n in enumerate(RUNS + RUNS[::-1]):
        pairs += [(read, 1)] * n
    tasks = check(exe, pairs)
    assert len(tasks) == 2 * sum((n + TASK - 1) // TASK for n in RUNS)
    # equal reads that do not touch are runs of their own
    tasks = check(exe, [(1, 1)] * 40 + [(2, 1)] * 40 + [(1, 1)] * 40)
    assert tasks == [(1, 0, 40), (2, 40, 40), (1, 80, 40)]


def test_a_gap_longer_than_a_task(exe):
    # tested, 200 untested, tested: two tasks of one pair, nothing in between
    assert check(exe, [(0, 1)] + [(0, 0)] * 200 + [(0, 1)]) == [(0, 0, 1), (0, 201, 1)]
    # a tested pair exactly 63 / 64 behind the first: one task / two
    assert check(exe, [(0, 1)] + [(0, 0)] * 62 + [(0, 1)]) == [(0, 0, 64)]
    assert check(exe, [(0, 1)] + [(0, 0)] * 63 + [(0, 1)]) == [(0, 0, 1), (0, 64, 1)]


def test_random_lists(exe):
    rng = random.Random(20)
    for _ in range(60):
        pairs = []
        for _ in range(rng.randint(0, 8)):
            read = rng.randrange(5)
            density = rng.choice([0.0, 0.05, 0.5, 1.0])
            pairs += [(read, rng.random() < density) for _ in range(rng.choice(RUNS + [2, 33, 200]))]
        check(exe, pairs)
