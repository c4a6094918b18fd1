"""CPU: the pair rule of the device-built invariance graph (isocon_amd/csrc/end_inv_core.hpp) compiled with g++ into a program of its own
(tests/emul/end_inv_emul.cpp), a second time with -fsanitize=undefined,address: the program packs the sequences into a plane array of
exactly nchunks * n * 2 words, as the store does, and runs the rule over every window pair; its rows against
end_invariant_functions._pair_is_invariant over the same windows (tests/end_inv_cases.py)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import end_inv_cases as EC  # noqa: E402

SRC = os.path.join(HERE, "emul", "end_inv_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "hw_graph_core.hpp", "end_inv_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request):
    exe = os.path.join(HERE, "emul", "_end_inv_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def run(exe, seqs, thr):
    """(rows, counters) of the program"""
    done = subprocess.run([exe, str(thr)], input="%d\n%s\n" % (len(seqs), "\n".join(seqs)), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = done.stdout.splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:-1]]
    assert [r[0] for r in rows] == list(range(len(seqs))) and lines[-1].startswith("#")
    return [r[1:] for r in rows], dict(zip(("pairs", "survivors", "verified", "invariant"), (int(x) for x in lines[-1].split()[1:])))


def check(exe, seqs, thr):
    rows, ctr = run(exe, seqs, thr)
    expect, pairs = EC.expected_rows(seqs, thr)
    assert rows == expect
    assert ctr["pairs"] == pairs and ctr["invariant"] == sum(len(r) for r in expect)
    assert ctr["invariant"] <= ctr["verified"] <= min(ctr["survivors"], ctr["pairs"])
    return ctr


@pytest.mark.parametrize("thr", EC.THRS)
def test_directed_cases_equal_pair_is_invariant(prog, thr):
    invariant = surviving_misses = 0
    for name, seqs, t in EC.directed_cases():
        if t == thr:
            ctr = check(prog, seqs, thr)
            invariant += ctr["invariant"]
            surviving_misses += ctr["verified"] - ctr["invariant"]
    print("thr %d: %d invariant pairs, %d verified pairs that are not" % (thr, invariant, surviving_misses))
    assert invariant >= 10 and surviving_misses >= 10          # (both verdicts of the full verification occur)


@pytest.mark.parametrize("thr", EC.THRS)
def test_planted_mismatch_removes_the_edge(prog, thr):
    seqs, A, good, bad = EC.planted_mismatches(thr)
    rows, _ = run(prog, seqs, thr)
    assert len(bad) >= 2 * len(good) and len(good) >= 1
    assert {seqs[p] for p in rows[seqs.index(A)]} == set(good) - {A}          # (thr 0, 1: the contained partner is A itself)


@pytest.mark.parametrize("thr", [t for t in EC.THRS if t >= 2])
def test_first_occurrence_decides(prog, thr):
    A, fails, passes = EC.first_occurrence_pair(thr)
    rows, _ = run(prog, EC.by_length([A, fails, passes]), thr)
    seqs = EC.by_length([A, fails, passes])
    assert [seqs[p] for p in rows[seqs.index(A)]] == [passes]
    assert A[2:2 + len(fails)] == fails and fails in A[:len(fails)]          # (it occurs again, at a shift that would pass)


@pytest.mark.parametrize("name", sorted(EC.RANDOM_FAMILIES))
def test_random_families_equal_pair_is_invariant(prog, name):
    seqs, thr = EC.RANDOM_FAMILIES[name]()
    ctr = check(prog, seqs, thr)
    assert ctr["invariant"] >= 50 and ctr["verified"] - ctr["invariant"] >= 50
    if name == "family_400_thr15":
        assert ctr["invariant"] > 100
