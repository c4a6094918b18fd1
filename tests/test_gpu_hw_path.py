"""GPU: infix ("HW") alignment paths for pair lists (isocon_hw_path_pairs / SeqStore.hw_path_pairs, the windowed instance of
csrc/nw_path.hpp) against the oracle (oracle.hw_path: hw_locate, then the full matrix of nw_path on t[start..end]), and
edlib_alignment_module.edlib_traceback_infix on top of it.  The shapes are the smallest at which the window code can go wrong: text
words are 32 bits, plane chunks and row blocks 64, walk requests 64 columns."""
import ctypes
import random
import re

import numpy as np
import pytest

from oracle import oracle as O
from test_nw_path_core import QLENS, mutate, rnd

pytestmark = pytest.mark.gpu

E_ARG, E_ALPHABET, E_CAPACITY, E_UNSUPPORTED = -1, -2, -4, -6
STARTS = [0, 1, 31, 32, 33, 63, 64, 65, 97]
FLANKS = [0, 1, 70]
_EXPECT = {}


def expect(q, t, k=-1):
    """the oracle's (row, [(length, op)]) under threshold k (negative: unbounded), computed once per case and shared by the tests;
    row = distance, start, end, leading / trailing insertion run -- all -1, 0, 0 and no path above k or with an empty sequence"""
    k = -1 if k is None or k < 0 else int(k)
    if (q, t, k) not in _EXPECT:
        r = O.hw_path(q, t, k) if q and t else {"cigar": None}
        if r["cigar"] is None:
            _EXPECT[(q, t, k)] = ([-1, -1, -1, 0, 0], [])
        else:
            path = [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", r["cigar"])]
            (start, end), = r["locations"]
            lead = path[0][0] if path[0][1] == "I" else 0
            trail = path[-1][0] if path[-1][1] == "I" else 0
            _EXPECT[(q, t, k)] = ([r["editDistance"], start, end, lead, trail], path)
    return _EXPECT[(q, t, k)]


def store_of(pairs):
    from isocon_amd.store import SeqStore
    seqs = sorted({s for p in pairs for s in p})
    index = {s: i for i, s in enumerate(seqs)}
    return SeqStore(seqs), [index[q] for q, _ in pairs], [index[t] for _, t in pairs]


def decoded(ops, ops_ptr, p):
    return [(int(o) >> 4, "=XID"[int(o) & 15]) for o in ops[int(ops_ptr[p]):int(ops_ptr[p + 1])]]


def check_path(q, row, path):
    """what holds for every infix path, whatever the oracle says"""
    ed, start, end, lead, trail = row
    n = {c: sum(l for l, o in path if o == c) for c in "=XID"}
    assert n["="] + n["X"] + n["I"] == len(q)
    assert n["="] + n["X"] + n["D"] == end - start + 1
    assert n["X"] + n["I"] + n["D"] == ed
    assert all(a[1] != b[1] for a, b in zip(path, path[1:])) and all(l > 0 for l, _ in path)
    assert path[0][1] != "D" and path[-1][1] != "D"
    assert lead == (path[0][0] if path[0][1] == "I" else 0) and trail == (path[-1][0] if path[-1][1] == "I" else 0)
    assert path[0][1] != "I" or start == 0


def check_list(pairs, k, rows, ops, ops_ptr):
    """every pair of the list against the oracle under its threshold; returns (hits, misses)"""
    assert rows.shape == (len(pairs), 5) and len(ops_ptr) == len(pairs) + 1 and int(ops_ptr[0]) == 0 and int(ops_ptr[-1]) == len(ops)
    hits = misses = 0
    for p, (q, t) in enumerate(pairs):
        e_row, e_path = expect(q, t, None if k is None else k[p])
        assert rows[p].tolist() == e_row, (q, t, p)
        path = decoded(ops, ops_ptr, p)
        assert path == e_path, (q, t, p)
        if e_row[0] < 0:
            misses += 1
            continue
        check_path(q, rows[p].tolist(), path)
        hits += 1
    return hits, misses


def window_cases():
    """every query length with every window offset and right flank: the query is an edited copy (0-6 edits, some at either end) of
    the bases planted behind a random left flank"""
    out = []
    for qlen in QLENS:
        rng = random.Random(7000 + qlen)
        for i, (start, flank) in enumerate((s, f) for s in STARTS for f in FLANKS):
            core = rnd(rng, qlen)
            nmut = (i + qlen) % 7
            q = mutate(rng, core, nmut, ends=nmut >= 2 and nmut % 2 == 0) or "A"
            out.append((q, rnd(rng, start) + core + rnd(rng, flank)))
    return out


def border_cases():
    """queries that overhang their target on the left / on the right (leading / trailing I runs of 5, 70 and 140, longer than a walk
    request), an exon-sized D run inside the window, a query longer than its target"""
    rng = random.Random(12)
    core = rnd(rng, 60).replace("A", "C")
    tail = rnd(rng, 40).replace("A", "G")
    out = []
    for junk in (5, 70, 140):
        out += [("A" * junk + core, core + tail), (core + "A" * junk, tail + core)]
    a, b, exon = rnd(rng, 400).replace("A", "C"), rnd(rng, 400).replace("A", "G"), "A" * 130          # (no base of the exon matches by chance: one run)
    out.append((a + b, rnd(rng, 45) + a + exon + b + rnd(rng, 30)))
    q = rnd(rng, 150)
    out.append((q, mutate(rng, q[40:130], 3)))
    return out


def two_pass_case():
    rng = random.Random(4097)
    core = rnd(rng, 4097)
    return mutate(rng, core, 6), rnd(rng, 33) + core + rnd(rng, 170)


def workload_cases():
    """the workload's own shape: a 2.4 kb slice of a 2.5 kb read, with ~40 edits, inside the read"""
    rng = random.Random(2400)
    out = []
    for i in range(5):
        read = rnd(rng, 2500)
        a = rng.randint(20, 80)
        out.append((mutate(rng, read[a:a + 2400], 40), read))
    return out


def trace_bytes(m, ms):
    """hwf_trace_units (csrc/hw_full_core.hpp) x 16"""
    blocks = (m + 63) // 64
    last = (blocks + 63) // 64 - 1
    r32 = lambda u: (u + 31) & ~31
    lanes = blocks - 64 * last
    return 16 * (r32((blocks + 1) // 2) + last * r32((ms + 63) * 64) + r32((ms + lanes - 1) * lanes))


@pytest.fixture(scope="module")
def window_list():
    pairs = window_cases()
    st, a, b = store_of(pairs)
    yield pairs, st, a, b
    st.close()


def test_window_offsets(window_list):
    pairs, st, a, b = window_list
    rows, ops, ops_ptr = st.hw_path_pairs(a, b)
    assert check_list(pairs, None, rows, ops, ops_ptr) == (len(pairs), 0)
    assert rows.tolist() == st.hw_pairs(a, b, [len(q) for q, _ in pairs], wide=True).tolist()
    # the cases are what they are meant to be: every offset under every query length of a block or more, paths with edits
    for qlen in QLENS[2:]:
        seen = {int(rows[p, 1]) for p, (q, _) in enumerate(pairs) if abs(len(q) - qlen) <= 6}
        assert seen >= set(STARTS), (qlen, seen)
    assert sum(int(r[0]) > 0 for r in rows) >= 150 and sum(int(r[3]) > 0 for r in rows) >= 1 and sum(int(r[4]) > 0 for r in rows) >= 1


@pytest.mark.parametrize("kmode", ["ed-1", "ed", "ed+1", "300"])
def test_threshold_modes(window_list, kmode):
    pairs, st, a, b = window_list
    d = np.array([expect(q, t)[0][0] for q, t in pairs])
    k = {"ed-1": d - 1, "ed": d, "ed+1": d + 1, "300": np.full_like(d, 300)}[kmode]
    rows, ops, ops_ptr = st.hw_path_pairs(a, b, k)
    hits, misses = check_list(pairs, k, rows, ops, ops_ptr)
    assert rows.tolist() == st.hw_pairs(a, b, np.where(k < 0, [len(q) for q, _ in pairs], k), wide=True).tolist()
    if kmode == "ed-1":
        assert misses == int((d > 0).sum()) >= 150 and hits == int((d == 0).sum())          # (k = -1 at distance 0 is unbounded: a hit)
        assert all(int(ops_ptr[p]) == int(ops_ptr[p + 1]) for p in range(len(pairs)) if d[p] > 0)
    else:
        # the same path whichever route located the window: the banded kernels here, the un-banded ones under k = 300
        assert misses == 0
        for p, (q, t) in enumerate(pairs):
            assert decoded(ops, ops_ptr, p) == expect(q, t)[1]


def test_border_runs_longer_than_a_request():
    pairs = border_cases()
    st, a, b = store_of(pairs)
    rows, ops, ops_ptr = st.hw_path_pairs(a, b)
    assert check_list(pairs, None, rows, ops, ops_ptr) == (len(pairs), 0)
    assert [int(r[3]) for r in rows[:6:2]] == [5, 70, 140] and [int(r[4]) for r in rows[1:6:2]] == [5, 70, 140]
    assert decoded(ops, ops_ptr, 6) == [(400, "="), (130, "D"), (400, "=")] and int(rows[6, 1]) == 45
    assert len(pairs[7][0]) > len(pairs[7][1]) and int(rows[7, 3]) > 0 and int(rows[7, 4]) > 0
    # ... and with every pair's own distance as the threshold (banded where that band fits)
    d = rows[:, 0].copy()
    again = st.hw_path_pairs(a, b, d)
    assert [x.tolist() for x in again] == [rows.tolist(), ops.tolist(), ops_ptr.tolist()]
    st.close()


@pytest.mark.parametrize("k", [10, 300])
def test_query_above_4096_rows(k):
    q, t = two_pass_case()
    st, a, b = store_of([(q, t)])
    rows, ops, ops_ptr = st.hw_path_pairs(a, b, k)
    assert check_list([(q, t)], [k], rows, ops, ops_ptr) == (1, 0)
    assert 0 < int(rows[0, 0]) <= 6 and int(rows[0, 1]) == 33
    st.close()


def test_list_mechanics():
    from isocon_amd.store import SeqStore
    rng = random.Random(9)
    core = rnd(rng, 150)
    q, t = mutate(rng, core, 5), rnd(rng, 40) + core + rnd(rng, 25)
    pairs = [(q, t)] * 70 + [(t, t), (core, t)]
    st, a, b = store_of(pairs)
    rows, ops, ops_ptr = st.hw_path_pairs(a, b, 8)
    assert check_list(pairs, [8] * 72, rows, ops, ops_ptr) == (72, 0)
    assert decoded(ops, ops_ptr, 70) == [(len(t), "=")] and rows[70].tolist() == [0, 0, len(t) - 1, 0, 0]
    assert decoded(ops, ops_ptr, 71) == [(150, "=")] and rows[71].tolist() == [0, 40, 189, 0, 0]
    st.close()
    # empty sequences: a row of -1 and no ops, between hits
    st = SeqStore(["", "ACG", "TTACGT"])
    rows, ops, ops_ptr = st.hw_path_pairs([1, 0, 1, 0, 1], [2, 1, 0, 0, 2], 2)
    assert rows.tolist() == [[0, 2, 4, 0, 0], [-1, -1, -1, 0, 0], [-1, -1, -1, 0, 0], [-1, -1, -1, 0, 0], [0, 2, 4, 0, 0]]
    assert ops_ptr.tolist() == [0, 1, 1, 1, 1, 2] and decoded(ops, ops_ptr, 4) == [(3, "=")]
    st.close()
    # no hit at all
    pairs = [(rnd(rng, 80), rnd(rng, 120)) for _ in range(5)]
    st, a, b = store_of(pairs)
    rows, ops, ops_ptr = st.hw_path_pairs(a, b, 3)
    assert (rows[:, 0] == -1).all() and len(ops) == 0 and ops_ptr.tolist() == [0] * 6
    st.close()


def raw_call(st, qa, ta, ka, cap):
    from isocon_amd import _lib
    p32, p64, pi = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)
    n = len(qa)
    rows = np.full((n, 5), -7, dtype=np.int32)
    ops = np.zeros(max(cap, 1), dtype=np.uint32)
    ptr = np.zeros(n + 1, dtype=np.uint64)
    needed = ctypes.c_uint64(0)
    rc = _lib.lib().isocon_hw_path_pairs(st.handle, qa.ctypes.data_as(p32), ta.ctypes.data_as(p32), ka.ctypes.data_as(pi), n, rows.ctypes.data_as(pi),
                                         ops.ctypes.data_as(p32) if cap else None, ptr.ctypes.data_as(p64), cap, ctypes.byref(needed), None)
    return rc, rows, ops, ptr, int(needed.value)


def test_capacity_protocol_and_errors():
    from isocon_amd.store import SeqStore
    pairs = [c for c in window_cases() if 60 <= len(c[0]) <= 70][:12] + [(rnd(random.Random(3), 64), rnd(random.Random(4), 90))]
    st, a, b = store_of(pairs)
    want = st.hw_path_pairs(a, b, 8)
    assert (want[0][:, 0] >= 0).sum() >= 10 and want[0][-1, 0] == -1
    qa, ta, ka = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32), np.full(len(pairs), 8, dtype=np.int32)
    rc, rows, _, ptr, needed = raw_call(st, qa, ta, ka, 0)
    assert rc == E_CAPACITY and needed == len(want[1]) > 0
    assert rows.tolist() == want[0].tolist() and ptr.tolist() == want[2].tolist()          # valid although nothing fitted
    rc, rows, _, ptr, needed2 = raw_call(st, qa, ta, ka, needed - 1)
    assert rc == E_CAPACITY and needed2 == needed and rows.tolist() == want[0].tolist() and ptr.tolist() == want[2].tolist()
    rc, rows, ops, ptr, needed2 = raw_call(st, qa, ta, ka, needed)
    assert rc == 0 and needed2 == needed
    assert (rows.tolist(), ops[:needed].tolist(), ptr.tolist()) == (want[0].tolist(), want[1].tolist(), want[2].tolist())
    bad = qa.copy()
    bad[3] = st.n
    assert raw_call(st, bad, ta, ka, needed)[0] == E_ARG
    neg = ka.copy()
    neg[2] = -1
    assert raw_call(st, qa, ta, neg, needed)[0] == E_ARG
    big = ka.copy()
    big[2] = (1 << 20) + 1
    assert raw_call(st, qa, ta, big, needed)[0] == E_UNSUPPORTED
    st.close()
    st = SeqStore(["ACGTNACGTTGCAACGT", "GGACGTACGTNGCAACGGTCC"])
    one = np.array([0, 1], dtype=np.uint32)
    assert raw_call(st, one[:1], one[1:], np.array([5], dtype=np.int32), 16)[0] == E_ALPHABET
    st.close()


def test_own_symbol_map():
    rng = random.Random(21)
    pairs = []
    for n in (30, 64, 130):
        core = "".join(rng.choice("acgu") for _ in range(n))
        v = list(core)
        for _ in range(3):
            v[rng.randrange(len(v))] = rng.choice("acgu")
        del v[rng.randrange(1, len(v) - 1)]
        flank = lambda m: "".join(rng.choice("acgu") for _ in range(m))
        pairs.append(("".join(v), flank(37) + core + flank(20)))
    st, a, b = store_of(pairs)
    rows, ops, ops_ptr = st.hw_path_pairs(a, b, 6)
    assert check_list(pairs, [6] * 3, rows, ops, ops_ptr) == (3, 0)
    st.close()


def test_trace_budget(monkeypatch):
    rng = random.Random(13)
    pairs = []
    for _ in range(9):
        core = rnd(rng, rng.randint(180, 220))
        pairs.append((mutate(rng, core, 4), rnd(rng, rng.randint(30, 300)) + core + rnd(rng, rng.randint(0, 300))))
    st, a, b = store_of(pairs)
    want = st.hw_path_pairs(a, b, 10)
    assert check_list(pairs, [10] * 9, *want) == (9, 0)
    # the store of a hit is that of its WINDOW, whatever the target's length.  A budget that holds the largest store of the list and
    # not two of the smallest: every pair is a launch of its own
    need = [trace_bytes(len(q), int(r[2]) - int(r[1]) + 1) for (q, _), r in zip(pairs, want[0])]
    assert max(need) < 2 * min(need) and max(need) < min(trace_bytes(len(q), len(t)) for q, t in pairs if len(t) > 400)
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % max(need))
    again = st.hw_path_pairs(a, b, 10)
    assert [x.tolist() for x in again] == [x.tolist() for x in want]
    # three pairs per launch
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % (3 * max(need)))
    again = st.hw_path_pairs(a, b, 10)
    assert [x.tolist() for x in again] == [x.tolist() for x in want]
    # and one byte less than the largest: that pair is refused, with its sizes
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % (max(need) - 1))
    with pytest.raises(RuntimeError, match="unsupported request.*needs %d bytes" % max(need)):
        st.hw_path_pairs(a, b, 10)
    st.close()


def test_workload_shapes():
    from isocon_amd import edlib_alignment_module as EAM
    pairs = workload_cases()
    st, a, b = store_of(pairs)
    unbounded = st.hw_path_pairs(a, b)
    assert check_list(pairs, None, *unbounded) == (5, 0)
    assert all(25 <= int(r[0]) <= 40 for r in unbounded[0])
    by_len = st.hw_path_pairs(a, b, [len(q) for q, _ in pairs])
    assert [x.tolist() for x in by_len] == [x.tolist() for x in unbounded]
    banded = st.hw_path_pairs(a, b, 60)
    assert [x.tolist() for x in banded] == [x.tolist() for x in unbounded]
    st.close()
    before = dict(EAM.TRACEBACK_INFIX_STATS)
    for q, t in pairs:
        row, path = expect(q, t)
        assert EAM.edlib_traceback_infix(q, t, k=60) == (row[0], [(row[1], row[2])], "".join("%d%s" % o for o in path))
        assert EAM.edlib_traceback_infix(q, t, k=row[0] - 1) == (-1, [], None)
    assert EAM.edlib_traceback_infix(pairs[0][0], pairs[0][1], k=None)[0] == expect(*pairs[0])[0][0]
    assert EAM.TRACEBACK_INFIX_STATS == {"device": before["device"] + 11}
    with pytest.raises(NotImplementedError):
        EAM.edlib_traceback(pairs[0][0], pairs[0][1], mode="HW")
