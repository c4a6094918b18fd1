"""GPU: global alignment paths for pair lists (isocon_ed_path_pairs / SeqStore.ed_path_pairs, csrc/nw_path.hpp) against the oracle's
full matrix (oracle.nw_path: from the end cell I, then D, then the diagonal), and the two Python callers on top of it
(edlib_alignment_module.edlib_traceback, end_invariant_functions.edlib_traceback_allow_ends)."""
import ctypes
import random

import numpy as np
import pytest

from conftest import golden
from oracle import oracle as O
from test_nw_path_core import QLENS, border_cases, length_cases, long_cases, mutate, rnd

pytestmark = pytest.mark.gpu

E_ARG, E_ALPHABET, E_CAPACITY, E_UNSUPPORTED = -1, -2, -4, -6
_EXPECT = {}


def expect(q, t):
    """the oracle's (distance, [(length, op)]), computed once per pair and shared by the tests"""
    if (q, t) not in _EXPECT:
        _EXPECT[(q, t)] = O.nw_path(q, t)
    return _EXPECT[(q, t)]


def store_of(pairs):
    from isocon_amd.store import SeqStore
    seqs = sorted({s for p in pairs for s in p})
    index = {s: i for i, s in enumerate(seqs)}
    return SeqStore(seqs), [index[q] for q, _ in pairs], [index[t] for _, t in pairs]


def decoded(ops, ops_ptr, p):
    return [(int(o) >> 4, "=XID"[int(o) & 15]) for o in ops[int(ops_ptr[p]):int(ops_ptr[p + 1])]]


def check_invariants(q, t, ed, path):
    n = {c: sum(l for l, o in path if o == c) for c in "=XID"}
    assert n["="] + n["X"] + n["I"] == len(q)
    assert n["="] + n["X"] + n["D"] == len(t)
    assert n["X"] + n["I"] + n["D"] == ed
    assert all(a[1] != b[1] for a, b in zip(path, path[1:]))
    assert all(l > 0 for l, _ in path)


def check_list(pairs, k, ed, ops, ops_ptr):
    """every pair of the list against the oracle under its threshold (None / negative: unbounded)"""
    assert len(ed) == len(pairs) and len(ops_ptr) == len(pairs) + 1 and int(ops_ptr[0]) == 0 and int(ops_ptr[-1]) == len(ops)
    hits = misses = 0
    for p, (q, t) in enumerate(pairs):
        e_ed, e_ops = expect(q, t)
        kp = None if k is None else int(k[p])
        if kp is not None and kp >= 0 and e_ed > kp:
            assert int(ed[p]) == -1 and int(ops_ptr[p]) == int(ops_ptr[p + 1]), (q, t, kp)          # dense across hits and misses
            misses += 1
            continue
        path = decoded(ops, ops_ptr, p)
        assert (int(ed[p]), path) == (e_ed, e_ops), (q, t, kp)
        check_invariants(q, t, e_ed, path)
        hits += 1
    return hits, misses


@pytest.fixture(scope="module")
def length_list():
    pairs = [c for n in QLENS for c in length_cases(n)] + border_cases()
    st, a, b = store_of(pairs)
    yield pairs, st, a, b
    st.close()


@pytest.mark.parametrize("kmode", ["none", "0", "ed-1", "ed", "ed+1"])
def test_lengths_against_oracle(length_list, kmode):
    pairs, st, a, b = length_list
    d = np.array([expect(q, t)[0] for q, t in pairs])
    k = {"none": None, "0": np.zeros_like(d), "ed-1": d - 1, "ed": d, "ed+1": d + 1}[kmode]
    ed, ops, ops_ptr = st.ed_path_pairs(a, b, k)
    hits, misses = check_list(pairs, k, ed, ops, ops_ptr)
    if kmode in ("0", "ed-1"):
        assert misses >= 50 and hits >= 5          # (k = ed - 1 = -1 at distance 0 is unbounded: a hit)
    else:
        assert misses == 0


def test_queries_above_4096_rows():
    pairs = long_cases()
    st, a, b = store_of(pairs)
    ed, ops, ops_ptr = st.ed_path_pairs(a, b)
    assert check_list(pairs, None, ed, ops, ops_ptr) == (2, 0)
    assert int(ops_ptr[2] - ops_ptr[1]) >= 200
    st.close()


def test_empty_sequences():
    from isocon_amd.store import SeqStore
    st = SeqStore(["", "ACG", "ACGT"])
    q, t = [0, 1, 0, 1, 0], [1, 0, 0, 2, 2]
    ed, ops, ops_ptr = st.ed_path_pairs(q, t)
    assert ed.tolist() == [3, 3, 0, 1, 4]
    assert [decoded(ops, ops_ptr, p) for p in range(5)] == [[(3, "D")], [(3, "I")], [], [(3, "="), (1, "D")], [(4, "D")]]
    ed, ops, ops_ptr = st.ed_path_pairs(q, t, [2, 3, 0, 0, -1])
    assert ed.tolist() == [-1, 3, 0, -1, 4]
    assert [decoded(ops, ops_ptr, p) for p in range(5)] == [[], [(3, "I")], [], [], [(4, "D")]]
    st.close()


def test_repeated_pair_and_equal_sequences():
    rng = random.Random(8)
    q = rnd(rng, 150)
    t = mutate(rng, q, 5)
    pairs = [(q, t)] * 70 + [(q, q)]
    st, a, b = store_of(pairs)
    ed, ops, ops_ptr = st.ed_path_pairs(a, b, 5)
    assert check_list(pairs, [5] * 71, ed, ops, ops_ptr) == (71, 0)
    assert decoded(ops, ops_ptr, 70) == [(150, "=")]
    st.close()


def test_capacity_protocol_and_bad_ids():
    from isocon_amd import _lib
    pairs = length_cases(65)
    st, a, b = store_of(pairs)
    want = st.ed_path_pairs(a, b)
    L, n = _lib.lib(), len(pairs)
    qa, ta = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    p32, p64, pi = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)

    def call(cap, qq=qa):
        ed = np.full(n, -7, dtype=np.int32)
        ops = np.zeros(max(cap, 1), dtype=np.uint32)
        ptr = np.zeros(n + 1, dtype=np.uint64)
        needed = ctypes.c_uint64(0)
        rc = L.isocon_ed_path_pairs(st.handle, qq.ctypes.data_as(p32), ta.ctypes.data_as(p32), None, n, ed.ctypes.data_as(pi),
                                    ops.ctypes.data_as(p32) if cap else None, ptr.ctypes.data_as(p64), cap, ctypes.byref(needed), None)
        return rc, ed, ops, ptr, int(needed.value)

    rc, ed, _, ptr, needed = call(0)
    assert rc == E_CAPACITY and needed == len(want[1]) > 0
    assert ed.tolist() == want[0].tolist() and ptr.tolist() == want[2].tolist()          # valid although nothing fitted
    assert call(needed - 1)[0] == E_CAPACITY
    rc, ed, ops, ptr, needed2 = call(needed)
    assert rc == 0 and needed2 == needed
    assert (ed.tolist(), ops[:needed].tolist(), ptr.tolist()) == (want[0].tolist(), want[1].tolist(), want[2].tolist())
    bad = qa.copy()
    bad[3] = st.n
    assert call(needed, bad)[0] == E_ARG
    st.close()


def trace_bytes(m, ms):
    """hwf_trace_units (csrc/hw_full_core.hpp) x 16"""
    blocks = (m + 63) // 64
    last = (blocks + 63) // 64 - 1
    r32 = lambda u: (u + 31) & ~31
    lanes = blocks - 64 * last
    return 16 * (r32((blocks + 1) // 2) + last * r32((ms + 63) * 64) + r32((ms + lanes - 1) * lanes))


def test_trace_budget(monkeypatch):
    rng = random.Random(13)
    pairs = []
    for _ in range(9):
        q = rnd(rng, rng.randint(180, 220))
        pairs.append((q, mutate(rng, q, 4)))
    st, a, b = store_of(pairs)
    want = st.ed_path_pairs(a, b)
    assert check_list(pairs, None, *want) == (9, 0)
    # a budget that holds the largest store of the list and not two of the smallest: every pair is a launch of its own
    need = [trace_bytes(len(q), len(t)) for q, t in pairs]
    assert max(need) < 2 * min(need)
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % max(need))
    again = st.ed_path_pairs(a, b)
    assert [x.tolist() for x in again] == [x.tolist() for x in want]
    # three pairs per launch
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % (3 * max(need)))
    again = st.ed_path_pairs(a, b)
    assert [x.tolist() for x in again] == [x.tolist() for x in want]
    # and one byte less than the largest: that pair is refused, with its sizes
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_trace_budget=%d" % (max(need) - 1))
    with pytest.raises(RuntimeError, match="unsupported request.*needs %d bytes" % max(need)):
        st.ed_path_pairs(a, b)
    st.close()


def test_own_symbol_map():
    rng = random.Random(21)
    pairs = []
    for n in (30, 64, 130):
        q = "".join(rng.choice("acgu") for _ in range(n))
        v = list(q)
        for _ in range(4):
            v[rng.randrange(len(v))] = rng.choice("acgu")
        del v[rng.randrange(len(v))]
        pairs.append((q, "".join(v)))
    st, a, b = store_of(pairs)
    ed, ops, ops_ptr = st.ed_path_pairs(a, b)
    assert check_list(pairs, None, ed, ops, ops_ptr) == (3, 0)
    st.close()


def test_more_than_four_symbols():
    from isocon_amd import _lib
    from isocon_amd import edlib_alignment_module as EAM
    from isocon_amd.store import SeqStore
    x, y = "ACGTNACGTTGCAACGT", "ACGTACGTNGCAACGGT"
    st = SeqStore([x, y])
    ed = np.zeros(1, dtype=np.int32)
    ptr = np.zeros(2, dtype=np.uint64)
    ids = np.array([0, 1], dtype=np.uint32)
    p32 = ctypes.POINTER(ctypes.c_uint32)
    rc = _lib.lib().isocon_ed_path_pairs(st.handle, ids[:1].ctypes.data_as(p32), ids[1:].ctypes.data_as(p32), None, 1, ed.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         None, ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 0, None, None)
    assert rc == E_ALPHABET
    st.close()
    e_ed, e_ops = expect(x, y)
    before = dict(EAM.TRACEBACK_STATS)
    assert EAM.edlib_traceback(x, y, k=10) == (e_ed, [(0, len(y) - 1)], "".join("%d%s" % o for o in e_ops))
    assert EAM.TRACEBACK_STATS == {"device": before["device"], "host": before["host"] + 1}


def test_edlib_traceback_on_reads_of_the_workload():
    """one related pair of 2 500 bases: beyond what the host route's Python matrix is for"""
    from isocon_amd import edlib_alignment_module as EAM
    rng = random.Random(2500)
    x = rnd(rng, 2500)
    y = mutate(rng, x, 30)
    e_ed, e_ops = expect(x, y)
    assert 10 <= e_ed <= 30
    before = dict(EAM.TRACEBACK_STATS)
    assert EAM.edlib_traceback(x, y, mode="NW", task="path", k=40) == (e_ed, [(0, len(y) - 1)], "".join("%d%s" % o for o in e_ops))
    assert EAM.TRACEBACK_STATS == {"device": before["device"] + 1, "host": before["host"]}
    assert EAM.edlib_traceback(x, y, mode="NW", task="path", k=e_ed - 1) == (-1, [], None)


def test_traceback_allow_ends_against_the_reference():
    from isocon_amd import end_invariant_functions as END
    g = golden("g21_traceback_allow_ends.json")
    assert len(g["cases"]) >= 40 and {c["end_threshold"] for c in g["cases"]} == {0, 5, 15}
    for c in g["cases"]:
        got = END.edlib_traceback_allow_ends(c["x"], c["y"], mode="NW", task="path", k=c["k"], end_threshold=c["end_threshold"])
        assert got == (c["ed"], [tuple(l) for l in c["locations"]], c["cigar"]), c
    with pytest.raises(NotImplementedError):
        END.edlib_traceback_allow_ends("ACGT", "ACGT", mode="HW")
