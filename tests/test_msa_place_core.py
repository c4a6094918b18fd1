"""CPU: the placement rule of the wide-slot insertions (isocon_amd/csrc/msa_place_core.hpp) compiled with g++ into a program of its own
(tests/emul/msa_place_emul.cpp), a second time with -fsanitize=undefined,address: the program places every pair on 64 emulated lanes the
way k_msa_place does, with the DP bytes in a heap array of exactly PLACE_DP_BYTES; its columns against functions.get_best_solution."""
import os
import subprocess
import sys
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msa_place_cases as PC  # noqa: E402

SRC = os.path.join(HERE, "emul", "msa_place_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "msa_place_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request):
    exe = os.path.join(HERE, "emul", "_msa_place_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def run(exe, mode, lines):
    done = subprocess.run([exe, mode], input="%d\n%s\n" % (len(lines), "\n".join(lines)), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    out = done.stdout.splitlines()
    assert len(out) == len(lines)
    return out


_EXPECTED = {}


def expected(name):
    """the pairs of a family with the anchor's columns and step, computed once for both builds of the program"""
    if name not in _EXPECTED:
        pairs = PC.exhaustive_pairs() if name == "exhaustive" else PC.random_pairs()
        _EXPECTED[name] = (pairs, [PC.anchor(rep, q) for rep, q in pairs])
    return _EXPECTED[name]


def compare(prog, name):
    pairs, want = expected(name)
    got = run(prog, "place", ["%s %s" % pq for pq in pairs])
    wrong = [(pq, g, w) for pq, g, w in zip(pairs, got, want) if g != "%s %d" % w]
    assert not wrong, wrong[:5]
    return Counter((len(rep), step) for (rep, _), (_, step) in zip(pairs, want))


def test_every_pair_up_to_four_bases(prog):
    pairs, _ = expected("exhaustive")
    assert len(pairs) == 16 * 20 + 64 * 84 + 256 * 340
    seen = compare(prog, "exhaustive")
    for step in (PC.SUBSTRING, PC.THREADED, PC.OFFSET, PC.LEFT):
        assert sum(n for (_, s), n in seen.items() if s == step) > 0, step
    assert seen[(3, PC.LEFT)] > 0 and seen[(4, PC.OFFSET)] > 0 and seen[(2, PC.THREADED)] > 0
    assert "".join(PC.anchor("AA", "C")[0]) == "C---"          # the pads take part as characters that match nothing


def test_random_pairs_around_the_word_and_lane_limits(prog):
    pairs, want = expected("random")
    assert {len(rep) for rep, _ in pairs} == set(PC.RANDOM_LONGEST)
    assert any(len(q) == 1 for _, q in pairs) and any(len(q) == len(rep) == 62 for rep, q in pairs)
    seen = compare(prog, "random")
    for n in PC.RANDOM_LONGEST:
        assert seen[(n, PC.THREADED)] >= 20 and seen[(n, PC.SUBSTRING)] >= 5, (n, seen)
    assert sum(n for (_, s), n in seen.items() if s in (PC.OFFSET, PC.LEFT)) >= 50


def test_the_representative_is_the_smallest_string(prog):
    sets = PC.representative_sets()
    got = run(prog, "rep", ["%d %s" % (len(s), " ".join(s)) for s in sets])
    assert got == [min(s) for s in sets]
    assert any(len(set(s)) == 1 for s in sets) and any(len({x[:32] for x in s}) == 1 and len(set(s)) > 1 for s in sets)
