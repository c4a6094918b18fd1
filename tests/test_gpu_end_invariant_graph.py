"""The invariance graph of the end-invariant collapse built on the device (isocon_end_invariant_graph, SeqStore.end_invariant_graph): the
reference's own outputs (tests/golden/g13_end_invariants.json) through the device route, the rows against the reference's test
(end_invariant_functions._pair_is_invariant) over the window for the directed cases of tests/end_inv_cases.py, the refusals, and the two
routes of the product functions against each other.  Every test checks that the device route ran (INVARIANT_STATS["device_calls"])."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import end_inv_cases as EC  # noqa: E402

G13 = json.load(open(os.path.join(HERE, "golden", "g13_end_invariants.json")))
pytestmark = pytest.mark.gpu


def params_of(thr):
    class Params(object):
        verbose = False
    Params.ignore_ends_len = thr
    return Params()


def device_rows(seqs, thr):
    """(rows, counters) of a length-sorted list through the product's own device call; fails where that call did not run"""
    from isocon_amd import end_invariant_functions as END
    before = END.INVARIANT_STATS["device_calls"]
    got = END._device_invariant_rows(list(seqs), thr)
    assert got is not None and END.INVARIANT_STATS["device_calls"] == before + 1
    row_ptr, cols, ctr = got
    assert len(row_ptr) == len(seqs) + 1 and row_ptr[0] == 0 and row_ptr[-1] == len(cols)
    return [cols[row_ptr[i]:row_ptr[i + 1]] for i in range(len(seqs))], ctr


def check_rows(seqs, thr):
    rows, ctr = device_rows(seqs, thr)
    expect, pairs = EC.expected_rows(seqs, thr)
    assert rows == expect
    assert ctr["pairs"] == pairs and ctr["invariant"] == sum(len(r) for r in expect)
    assert ctr["invariant"] <= ctr["verified"] <= min(ctr["survivors"], ctr["pairs"])
    return ctr


def host_variant(monkeypatch):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", (saved + "," if saved else "") + "inv_host_graph")


def graph_of(G):
    return list(G.nodes(data=True)), list(G.edges())


# ---- the reference's outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G13["cases"], ids=[c["name"] for c in G13["cases"]])
def test_reference_fixtures(case):
    from isocon_amd import end_invariant_functions as END
    before = END.INVARIANT_STATS["device_calls"]
    part = END.collapse_candidates_under_ends_invariant(dict(case["C"]), dict(case["support"]), params_of(case["ignore_ends_len"]))
    assert END.INVARIANT_STATS["device_calls"] == before + 1
    assert sorted([c, sorted(m)] for c, m in part.items()) == case["expect"]


# ---- the rows against the host rule ----------------------------------------------------------------------------------------------
DIRECTED = EC.directed_cases()


@pytest.mark.parametrize("case", DIRECTED, ids=[c[0] for c in DIRECTED])
def test_directed_cases_equal_pair_is_invariant(case):
    name, seqs, thr = case
    check_rows(seqs, thr)


@pytest.mark.parametrize("thr", EC.THRS)
def test_planted_mismatch_removes_the_edge(thr):
    seqs, A, good, bad = EC.planted_mismatches(thr)
    rows, _ = device_rows(seqs, thr)
    assert len(bad) >= 2 * len(good) and len(good) >= 1
    assert {seqs[p] for p in rows[seqs.index(A)]} == set(good) - {A}          # (thr 0, 1: the contained partner is A itself)


@pytest.mark.parametrize("thr", [t for t in EC.THRS if t >= 2])
def test_first_occurrence_decides(thr):
    A, fails, passes = EC.first_occurrence_pair(thr)
    seqs = EC.by_length([A, fails, passes])
    rows, _ = device_rows(seqs, thr)
    assert [seqs[p] for p in rows[seqs.index(A)]] == [passes]
    assert A[2:2 + len(fails)] == fails and A.find(fails) == 0          # (it occurs again, at a shift that would pass)


@pytest.mark.parametrize("name", sorted(EC.RANDOM_FAMILIES))
def test_random_families_equal_pair_is_invariant(name):
    seqs, thr = EC.RANDOM_FAMILIES[name]()
    ctr = check_rows(seqs, thr)
    # the verification kernel is not tested on nothing: pairs it rejects after the first-word test let them through
    assert ctr["invariant"] >= 50 and ctr["verified"] - ctr["invariant"] >= 50
    if name == "family_400_thr15":
        assert ctr["invariant"] > 100


def test_more_survivors_than_the_first_list_holds():
    """a periodic set: every pair survives at half of its shifts, the screen runs a second time with the room it counted"""
    seqs = EC.first_occurrence(15)
    ctr = check_rows(seqs, 15)
    assert ctr["survivors"] > ctr["pairs"] + 1024


def test_tiny_stores():
    from isocon_amd.store import SeqStore
    s = EC.rnd(__import__("random").Random(3), 90)
    for seqs in ([s], [s[:70], s], [s[:50], s], [s, s]):
        check_rows(EC.by_length(seqs), 15)
    st = SeqStore([])
    try:
        row_ptr, cols = st.end_invariant_graph(15)
        assert row_ptr.tolist() == [0] and len(cols) == 0
    finally:
        st.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def raw_call(st, thr, cap):
    from isocon_amd import _lib
    row_ptr = np.full(st.n + 1, 7, dtype=np.uint64)
    cols = np.zeros(max(cap, 1), dtype=np.uint32)
    ctr = np.zeros(4, dtype=np.uint64)
    needed = ctypes.c_uint64(0)
    rc = _lib.lib().isocon_end_invariant_graph(st.handle, thr, row_ptr.ctypes.data_as(_lib.u64p), cols.ctypes.data_as(_lib.u32p), cap, ctypes.byref(needed),
                                               ctr.ctypes.data_as(_lib.u64p), None)
    return rc, int(needed.value), row_ptr, cols, ctr


def test_capacity():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    seqs, thr = EC.RANDOM_FAMILIES["family_small_thr5"]()
    rows, ctr = device_rows(seqs, thr)
    n_edges = sum(len(r) for r in rows)
    row_ptr = np.cumsum([0] + [len(r) for r in rows])
    st = SeqStore(seqs)
    try:
        for cap in (0, n_edges - 1):
            rc, needed, got_ptr, _, got_ctr = raw_call(st, thr, cap)
            assert rc == _lib.ISOCON_E_CAPACITY and needed == n_edges and (got_ptr.astype(np.int64) == row_ptr).all()
            assert got_ctr.tolist() == [ctr["pairs"], ctr["survivors"], ctr["verified"], ctr["invariant"]]
        rc, needed, got_ptr, cols, _ = raw_call(st, thr, n_edges)
        assert rc == _lib.ISOCON_OK and needed == n_edges and cols.tolist() == [p for r in rows for p in r]
        # the wrapper grows its room once (4 n to begin with)
        dense = SeqStore([seqs[0]] * 40)          # (every pair of 40 equal sequences: 1 560 edges, more than max(4 n, 1 024))
        try:
            row_ptr2, cols2 = dense.end_invariant_graph(thr)
            assert row_ptr2.tolist() == [39 * i for i in range(41)] and cols2.tolist() == [p for i in range(40) for p in range(40) if p != i]
        finally:
            dense.close()
    finally:
        st.close()


def test_refusals_and_the_host_answer(monkeypatch):
    """a fifth symbol, a sequence of at most thr symbols: the raw entry refuses, the public function answers through the host route with the
    host's result; an unsorted store and a negative thr: ISOCON_E_ARG"""
    from isocon_amd import _lib
    from isocon_amd import end_invariant_functions as END
    from isocon_amd.store import SeqStore
    seqs, thr = EC.RANDOM_FAMILIES["family_small_thr5"]()
    rows, _ = device_rows(seqs, thr)          # (the device route runs in this process)
    C = {"c%d" % i: s for i, s in enumerate(seqs[:40])}
    sup = {a: 1 + i % 3 for i, a in enumerate(C)}
    fifth = dict(C, c3=C["c3"][:50] + "N" + C["c3"][51:])
    short = dict(C, extra=seqs[0][:thr], extra2=seqs[0][:thr + 1])
    for bad, status, text in ((fifth, _lib.ISOCON_E_ALPHABET, "more than four distinct symbols"), (short, _lib.ISOCON_E_UNSUPPORTED, "not longer than thr")):
        st = SeqStore(EC.by_length(list(bad.values())))
        try:
            rc = raw_call(st, thr, 10000)[0]
            assert rc == status and text in _lib.lib().isocon_last_error().decode()
        finally:
            st.close()
        before = dict(END.INVARIANT_STATS)
        bad_sup = {a: sup.get(a, 1) for a in bad}
        got = END.get_invariants_under_ignored_edge_ends_speed(bad, bad_sup, params_of(thr))
        assert END.INVARIANT_STATS == before          # (answered by the host)
        expect = set()
        for a1, s1 in bad.items():
            for a2, s2 in bad.items():
                if a1 != a2 and len(s1) - 2 * thr <= len(s2) <= len(s1) and END._pair_is_invariant(s1, s2, thr):
                    expect |= {(a1, a2), (a2, a1)}
        assert set(got.edges()) == expect and len(expect) > 10
    st = SeqStore(seqs[::-1])
    try:
        assert raw_call(st, thr, 10000)[0] == _lib.ISOCON_E_ARG
    finally:
        st.close()
    st = SeqStore(seqs)
    try:
        assert raw_call(st, -1, 10000)[0] == _lib.ISOCON_E_ARG
        assert raw_call(st, 1025, 10000)[0] == _lib.ISOCON_E_UNSUPPORTED
        rc, _, row_ptr, cols, _ = raw_call(st, thr, 10000)          # the store serves on
        assert rc == _lib.ISOCON_OK and cols[:int(row_ptr[-1])].tolist() == [p for r in rows for p in r]
    finally:
        st.close()


# ---- the two routes of the product -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["family_400", "equal_accessions"])
def test_routes_build_the_same_graph(name, monkeypatch):
    from isocon_amd import end_invariant_functions as END
    if name == "family_400":
        C = EC.family_400(1)
    else:          # two accessions of one sequence, inserted in an order that is not the length order
        seqs = EC.equal_runs(15)
        C = {"e%d" % i: s for i, s in enumerate(seqs[::-1])}
    sup = {a: 1 + i % 3 for i, a in enumerate(C)}
    before = dict(END.INVARIANT_STATS)
    G_dev = END.get_invariants_under_ignored_edge_ends_speed(C, sup, params_of(15))
    part_dev = END.collapse_candidates_under_ends_invariant(C, sup, params_of(15))
    assert END.INVARIANT_STATS["device_calls"] == before["device_calls"] + 2
    assert END.INVARIANT_STATS["edges"] > before["edges"] and END.INVARIANT_STATS["pairs"] > before["pairs"]
    assert END.INVARIANT_STATS["kernel_ms"] > before["kernel_ms"]
    host_variant(monkeypatch)
    middle = dict(END.INVARIANT_STATS)
    G_host = END.get_invariants_under_ignored_edge_ends_speed(C, sup, params_of(15))
    part_host = END.collapse_candidates_under_ends_invariant(C, sup, params_of(15))
    assert END.INVARIANT_STATS == middle          # (the switch keeps the calls on the host)
    assert graph_of(G_dev) == graph_of(G_host) and G_dev.number_of_edges() > 20
    assert part_dev == part_host and [(k, sorted(v)) for k, v in part_dev.items()] == [(k, sorted(v)) for k, v in part_host.items()]
