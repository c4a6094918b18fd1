"""CPU: the lane routines of the depth-limited 2-set search (isocon_amd/csrc/nn2_depth_core.hpp, shared host/device header) driven
round by round through tests/emul/nn2_depth_emul.cpp (g++): speculate with the threshold frozen, distances from the oracle with that
threshold, replay with the live state.  The rows must equal the oracle's restatement of the reference loop (orc_nn_2set with its
depth rule), order included, for every depth and every round size B."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emul", "_nn2_depth_emul.so")
SRC = os.path.join(HERE, "emul", "nn2_depth_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "nn2_depth_core.hpp")]

LANE = np.dtype([("a", np.uint32), ("b", np.uint32), ("best", np.int32), ("processed", np.uint32), ("flags", np.uint32)])
DEPTHS = [0, 1, 2, 3, 7, 50]
ROUND_SIZES = [1, 4, 32]


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def emul(request):
    so = SO if request.param == "plain" else SO.replace(".so", "_ubsan.so")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-static-libubsan"]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.nn2_emul_speculate.restype = ctypes.c_int64
    L.nn2_emul_replay.restype = ctypes.c_int64
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def walk_rows(L, seqs, is_t, depth, B):
    """rows of the batched scheme as {read: ([targets], best)} and the number of distances it asked for"""
    n = len(seqs)
    is_t = np.asarray(is_t, dtype=bool)
    lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
    assert np.all(np.diff(lens) >= 0)
    tpos = np.nonzero(is_t)[0].astype(np.uint32)
    qidx = np.nonzero(~is_t)[0].astype(np.uint32)
    tiq = np.searchsorted(tpos, qidx).astype(np.uint32)
    nq, nt = len(qidx), len(tpos)
    lanes = np.zeros(max(nq, 1), dtype=LANE)
    lanes["best"][:nq] = lens[qidx]
    jend = np.zeros(max(nq, 1), np.uint32); pbase = np.zeros_like(jend); pcnt = np.zeros_like(jend)
    cap = max(nq, 1) * (B + 1)
    pa = np.zeros(cap, np.uint32); pb = np.zeros(cap, np.uint32); pk = np.zeros(cap, np.int32)
    hits = np.zeros((max(nq, 1) * (nt + 1), 3), np.int32)
    n_hits = ctypes.c_uint64(0)
    tp = tpos if nt else np.zeros(1, np.uint32)
    asked = 0
    for _ in range(10 * (n + 2)):
        np_ = L.nn2_emul_speculate(_p(lens), _p(tp), nt, depth, B, nq, _p(qidx), _p(tiq), _p(lanes), _p(jend), _p(pbase), _p(pcnt), _p(pa), _p(pb), _p(pk),
                                   ctypes.c_uint64(cap))
        assert np_ >= 0
        assert int(pcnt[:nq].max(initial=0)) <= B + 1
        pd = O.ed_pairs(seqs, pa[:np_].astype(np.int32), pb[:np_].astype(np.int32), pk[:np_]) if np_ else np.zeros(0, np.int32)
        pd = np.ascontiguousarray(np.concatenate([pd, np.zeros(1, np.int32)]))
        asked += int(np_)
        open_ = L.nn2_emul_replay(_p(lens), _p(tp), nt, depth, nq, _p(qidx), _p(tiq), _p(lanes), _p(jend), _p(pbase), _p(pcnt), _p(pb), _p(pd),
                                  _p(hits), ctypes.c_uint64(len(hits)), ctypes.byref(n_hits))
        assert open_ >= 0, "replay reported %d" % open_
        if open_ == 0:
            break
    else:
        raise AssertionError("the rounds do not end")
    rows = {int(q): [] for q in qidx}
    best = {int(q): int(lanes["best"][r]) for r, q in enumerate(qidx)}
    for e, o, d in hits[:n_hits.value].tolist():
        if d == best[e]:
            rows[e].append(o)
    return rows, best, asked


def check(L, seqs, is_t, depth, B):
    n = len(seqs)
    row_ptr, cols, eds, calls = O.nn_2set(seqs, np.asarray(is_t, dtype=np.uint8), 0, n, depth)
    rows, best, asked = walk_rows(L, seqs, is_t, depth, B)
    n_reads = 0
    for i in range(n):
        want = cols[row_ptr[i]:row_ptr[i + 1]].tolist()
        if is_t[i]:
            assert not want and i not in rows
            continue
        n_reads += 1
        assert rows[i] == want, (i, depth, B, rows[i], want)
        if want:
            assert set(eds[row_ptr[i]:row_ptr[i + 1]].tolist()) == {best[i]}
    # every alignment of the reference was asked for; what speculation wastes is bounded per read (the round in which a side stops, the last round)
    assert calls <= asked <= calls + 3 * (B + 1) * max(n_reads, 1)
    return sum(len(r) for r in rows.values())


def _mutate(rng, s, nmut):
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


def random_set(rng, n, share):
    bases = ["".join(rng.choice("ACGT") for _ in range(rng.randint(12, 40))) for _ in range(4)]
    seqs = [_mutate(rng, rng.choice(bases), rng.choice([0, 0, 1, 1, 2, 3, 6])) for _ in range(n)]
    flags = [rng.random() < share for _ in range(n)]
    order = sorted(range(n), key=lambda i: len(seqs[i]))
    return [seqs[i] for i in order], [flags[i] for i in order]


@pytest.mark.parametrize("share", [0.02, 0.5, 0.9])
@pytest.mark.parametrize("B", ROUND_SIZES)
def test_random_sets_equal_oracle(emul, share, B):
    rng = random.Random(int(share * 100) * 7 + B)
    edges = 0
    for _ in range(6):
        seqs, flags = random_set(rng, rng.randint(30, 90), share)
        for depth in DEPTHS:
            edges += check(emul, seqs, flags, depth, B)
    assert edges > 0


@pytest.mark.parametrize("B", ROUND_SIZES)
def test_runs_of_equal_lengths(emul, B):
    rng = random.Random(11 + B)
    base = "".join(rng.choice("ACGT") for _ in range(24))
    seqs = []
    for _ in range(50):
        v = list(base)
        for _ in range(rng.choice([0, 1, 1, 2, 4])):
            v[rng.randrange(len(v))] = rng.choice("ACGT")          # substitutions only: one run of 50 equal lengths
        seqs.append("".join(v))
    seqs += [base + "AC"] * 1 + [_mutate(rng, base, 1)[:23].ljust(23, "A") for _ in range(10)]
    seqs.sort(key=len)
    flags = [rng.random() < 0.4 for _ in seqs]
    for depth in DEPTHS:
        check(emul, seqs, flags, depth, B)


@pytest.mark.parametrize("B", ROUND_SIZES)
def test_reads_at_both_ends_duplicates_and_empty_rows(emul, B):
    rng = random.Random(3)
    iso = "".join(rng.choice("ACGT") for _ in range(30))
    far = "".join(rng.choice("ACGT") for _ in range(30))
    seqs = ["AAA",                      # read, first entry: no target within len(read) -> both sides stop at once, empty row
            "CCCC",                     # read next to a target of its length + 1 that shares nothing: d = 5 > 4, empty row
            "GGGGG",                    # target
            iso[:29],                   # read
            iso,                        # target
            iso,                        # read: an exact duplicate of a target (d = 0)
            _mutate(rng, iso, 2).ljust(30, "T")[:30],          # read
            far,                        # target
            far[:15] + iso[15:],        # read
            iso + "ACGTAC",             # target
            iso + "ACGTACG"]            # read, last entry
    flags = [False, False, True, False, True, False, False, True, False, True, False]
    assert [len(s) for s in seqs] == sorted(len(s) for s in seqs)
    for depth in DEPTHS:
        check(emul, seqs, flags, depth, B)
    rows, best, _ = walk_rows(emul, seqs, flags, 50, B)
    assert rows[0] == [] and rows[1] == [] and rows[5] == [4] and best[5] == 0
    # the same list with the roles swapped: targets at both ends
    for depth in DEPTHS:
        check(emul, seqs, [not f for f in flags], depth, B)


@pytest.mark.parametrize("B", ROUND_SIZES)
def test_no_target_at_all(emul, B):
    rng = random.Random(5)
    seqs, _ = random_set(rng, 20, 0.0)
    for depth in DEPTHS:
        assert check(emul, seqs, [False] * len(seqs), depth, B) == 0
    assert check(emul, seqs, [True] * len(seqs), 3, B) == 0          # ... and no read
