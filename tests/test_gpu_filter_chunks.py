"""GPU: the two block-filter kernels of the nearest-neighbour main pass (isocon_amd/csrc/nn_filter.hpp: k_nn_block_filter, k_nn_block_filter2),
launched as the main pass launches them (isocon_block_filter_chunks) on the designed chunks of tests/filter_chunk_cases.py, against the
restatement there: which pairs survive, where a chunk's survivors go (table chunk of its class, second pass, flat pairs) and every counter.
All comparisons are exact; the order inside a chunk and among the flat pairs is not defined, so they compare sorted.  tests/test_filter_chunk_cases.py
shows on the CPU that the cases sit on the edges they claim and that a wrong rule changes the expected answer."""
import functools
import random

import numpy as np
import pytest

from tests import filter_chunk_cases as F

pytestmark = pytest.mark.gpu

COUNTERS = ("f_chunks", "f_chunks_narrow", "n_small", "f_rejected", "f_rejected2", "f_listed", "f_narrow_listed", "f_tasks", "overflow")
NAMES = list(F.cases())


def _flat(call):
    return (np.array([o for o, _, w in call.chunks], dtype=np.uint32), np.array([n for _, n, _ in call.chunks], dtype=np.uint8),
            np.concatenate([[0], np.cumsum([len(w) for _, _, w in call.chunks])]).astype(np.uint64), np.concatenate([w for _, _, w in call.chunks]))


def _run_once(call, second):
    """the entry's answer in the restatement's form: sorted table chunks, sorted flat pairs, counters"""
    from isocon_amd.store import SeqStore
    st = SeqStore(call.seqs)
    try:
        owner, narrow, ptr, words = _flat(call)
        got = st.block_filter_chunks(call.thr, owner, narrow, ptr, words, call.kcap, call.list_min, second)
    finally:
        st.close()
    out = {k: got[k] for k in COUNTERS}
    out["chunks"] = sorted((nr, o, sorted(int(w) for w in ws)) for nr, o, ws in got["chunks"])
    out["flat"] = sorted(zip(got["pa"].tolist(), got["pb"].tolist()))
    return out


@functools.lru_cache(maxsize=None)
def _run(name, second):
    return _run_once(F.cases()[name], second)


@pytest.mark.parametrize("second", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_survivors_routes_and_counters(name, second):
    call, exp, got = F.cases()[name], F.expected(name, second), _run(name, second)
    print({k: (got[k], exp[k]) for k in COUNTERS})
    assert got["overflow"] == 0
    # the chunks left for the tables: class, owner, and the list words with their two flag bits
    assert [(nr, o, len(ws)) for nr, o, ws in got["chunks"]] == [(nr, o, len(ws)) for nr, o, ws in exp["chunks"]]
    assert got["chunks"] == exp["chunks"]
    assert got["flat"] == exp["flat"]
    for k in COUNTERS:
        assert got[k] == exp[k], k
    # every pair sent in is kept once or rejected once
    sent = sum(len(w) for _, _, w in call.chunks)
    table_pairs = [(o, w & F.INDEX_MASK) for _, o, ws in got["chunks"] for w in ws]
    kept = table_pairs + got["flat"]
    assert len(table_pairs) == got["f_listed"] and len(got["flat"]) == got["n_small"]
    assert len(kept) + got["f_rejected"] + got["f_rejected2"] == sent
    assert len(set(kept)) == len(kept)
    assert set(kept) <= {(o, int(w) & F.INDEX_MASK) for o, _, words in call.chunks for w in words}


@pytest.mark.parametrize("name", NAMES)
def test_a_second_run_gives_the_same_sets(name):
    for second in (1, 0):
        assert _run_once(F.cases()[name], second) == _run(name, second)


def test_argument_errors():
    """every refusal of the entry (all decided on the host, before anything is launched)"""
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    seqs = ["ACGTACGTACGTACGTACGTACGT", "ACGTACGTACGTTCGTACGTACGTAA", "TTGACGTACGTACGTACGTACGAAC"]
    st = SeqStore(seqs)
    thr = np.array([3, 2, 1], dtype=np.int32)

    def rc(thr=thr, owner=(0,), narrow=(0,), ptr=(0, 2), words=(1 | F.PARTNER_BIT, 2 | F.OWNER_BIT), kcap=64, list_min=32, second=1, caps=None):
        owner, narrow = np.asarray(owner, dtype=np.uint32), np.asarray(narrow, dtype=np.uint8)
        ptr, words = np.asarray(ptr, dtype=np.uint64), np.asarray(words, dtype=np.uint32)
        nc, total = len(owner), len(words)
        c_cap, l_cap, p_cap = caps or (nc, total, total)
        bufs = [np.zeros(max(nc, 1) + 4, dtype=t) for t in (np.uint32, np.uint32, np.uint64)] + [np.zeros(total + 4, dtype=np.uint32) for _ in range(3)]
        ctr = np.zeros(9, dtype=np.uint64)
        p = lambda a, t: a.ctypes.data_as(t)
        return st._L.isocon_block_filter_chunks(st.handle, p(thr, _lib.i32p), nc, p(owner, _lib.u32p), p(narrow, _lib.u8p), p(ptr, _lib.u64p), p(words, _lib.u32p), kcap, list_min,
                                                 second, p(bufs[0], _lib.u32p), p(bufs[1], _lib.u32p), p(bufs[2], _lib.u64p), c_cap, p(bufs[3], _lib.u32p), l_cap,
                                                 p(bufs[4], _lib.u32p), p(bufs[5], _lib.u32p), p_cap, p(ctr, _lib.u64p))
    try:
        assert rc() == _lib.ISOCON_OK
        assert rc(owner=(3,)) == _lib.ISOCON_E_ARG                                              # owner out of range
        assert rc(words=(1 | F.PARTNER_BIT, 3 | F.OWNER_BIT)) == _lib.ISOCON_E_ARG               # partner out of range
        assert rc(words=(1 | F.PARTNER_BIT, F.INDEX_MASK | F.OWNER_BIT)) == _lib.ISOCON_E_ARG
        assert rc(owner=(0, 1), narrow=(0, 1), ptr=(0, 2, 2)) == _lib.ISOCON_E_ARG                # a chunk of 0 pairs
        assert rc(ptr=(0, F.CHUNK_MAX + 1), words=[1 | F.PARTNER_BIT] * (F.CHUNK_MAX + 1)) == _lib.ISOCON_E_ARG          # more than the builder hands over
        assert rc(ptr=(0, F.CHUNK_MAX), words=[1 | F.PARTNER_BIT] * F.CHUNK_MAX) == _lib.ISOCON_OK
        assert rc(thr=np.array([3, 65, 1], dtype=np.int32)) == _lib.ISOCON_E_ARG
        assert rc(thr=np.array([3, -1, 1], dtype=np.int32)) == _lib.ISOCON_E_ARG
        assert rc(thr=np.array([3, 64, 0], dtype=np.int32)) == _lib.ISOCON_OK
        assert rc(narrow=(2,)) == _lib.ISOCON_E_ARG and rc(second=2) == _lib.ISOCON_E_ARG and rc(list_min=0) == _lib.ISOCON_E_ARG
        for caps in ((0, 2, 2), (1, 1, 2), (1, 2, 1)):                                          # a capacity below the worst case
            assert rc(caps=caps) == _lib.ISOCON_E_ARG
    finally:
        st.close()
    st = SeqStore(seqs + ["ACGTNACGTRACGTYACGTACGTACGT"])          # more than four symbols: no 2-bit planes
    try:
        assert rc(thr=np.array([3, 2, 1, 0], dtype=np.int32)) == -2          # ISOCON_E_ALPHABET
    finally:
        st.close()


def test_a_pair_the_filter_rejects_is_never_a_hit(monkeypatch):
    """The entry and the product: a read set on which the main pass's filter rejects pairs; at the graph's final thresholds every pair the
    kernels reject through the entry has an edit distance above its threshold."""
    from isocon_amd import synth
    from isocon_amd.store import SeqStore
    seqs = sorted(dict.fromkeys(synth.make_reads(700, 300, 2, seed=77)[1]), key=len)
    n = len(seqs)
    assert 600 < n <= F.CHUNK_MAX
    st = SeqStore(seqs)
    try:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nn_filter_one_pass")
        best, row_ptr, cols, stats = st.nn_graph()
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
        assert stats["pairs_block_rejected"] > 0
        lens = np.array([len(s) for s in seqs])
        thr = np.minimum(np.where(best >= 0, best, 64), np.minimum(lens, 64)).astype(np.int32)          # the per-entry threshold of the main pass: min(best, length, 64)
        owners = np.arange(0, n, 10, dtype=np.uint32)
        chunks = [np.delete(np.arange(n, dtype=np.uint32), o) | np.uint32(F.OWNER_BIT | F.PARTNER_BIT) for o in owners]
        ptr = np.concatenate([[0], np.cumsum([len(w) for w in chunks])]).astype(np.uint64)
        for second in (0, 1):
            got = st.block_filter_chunks(thr, owners, np.zeros(len(owners), np.uint8), ptr, np.concatenate(chunks), 64, 256, second)
            kept = {(o, int(w) & F.INDEX_MASK) for _, o, ws in got["chunks"] for w in ws} | set(zip(got["pa"].tolist(), got["pb"].tolist()))
            rejected = np.array([(o, y) for o in owners.tolist() for y in range(n) if y != o and (o, y) not in kept], dtype=np.uint32)
            assert len(rejected) == got["f_rejected"] + got["f_rejected2"] > 0 and (second == 0) == (got["f_rejected2"] == 0 and got["f_tasks"] == 0)
            d = st.ed_pairs(rejected[:, 0], rejected[:, 1], None)
            k = np.maximum(thr[rejected[:, 0]], thr[rejected[:, 1]])
            assert (d > k).all(), rejected[d <= k][:10]
    finally:
        st.close()


@pytest.mark.parametrize("kind,seed", [(kind, seed) for kind in ("edges", "lowc", "homo") for seed in (1, 2)])
def test_stress_slice(kind, seed, monkeypatch):
    """scripts/stress_filter.py with fixed seeds: the graph with the filter, without it and with one pass over tables whatever is left are the
    same graph, and it is the reference loop's (oracle) in every row"""
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    seqs = sorted(dict.fromkeys(F.STRESS_GENERATORS[kind](random.Random(seed))[:600]), key=len)
    assert 2 <= len(seqs) <= 600
    st = SeqStore(seqs)
    try:
        g1 = st.nn_graph()
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nn_no_block_filter")
        g0 = st.nn_graph()
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nn_filter_one_pass,nn_table_chunks=0")
        g2 = st.nn_graph()
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
    finally:
        st.close()
    assert g0[3]["pairs_block_rejected"] == 0
    for g in (g1, g2):
        assert all((a == b).all() for a, b in zip(g[:3], g0[:3]))
    rp, c, e, _ = O.nn_1set(seqs, np.zeros(len(seqs), np.uint8), 0, len(seqs))
    assert (np.asarray(rp) == g1[1]).all() and (np.asarray(c) == g1[2]).all()
