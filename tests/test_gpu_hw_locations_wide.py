"""GPU: isocon_hw_locations_wide (csrc/hw_rows.hpp, hw_loc_wide_host.inc) -- every best location of an infix pair, bands above 512
diagonals too -- on the designed inputs of tests/hw_locations_wide_cases.py and on a random list, through the C ABI and SeqStore:
distance, row pointers and every (start, end) of EVERY pair against the plain restatement (hw_locations_cases.restated), the route from
the call's stats, the first location against hw_pairs(wide=True), the call's protocol and the Python entries.
tests/test_hw_locations_wide_core.py shows on the CPU that the inputs are what they claim."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest

import hw_locations_wide_cases as W

pytestmark = pytest.mark.gpu

ROUTE_KEYS = {"w1": "rows_w1", "w2": "rows_w2", "w4": "rows_w4", "wave": "wave"}


@contextmanager
def variant(value):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    os.environ["ISOCON_DEBUG_VARIANT"] = (saved + "," if saved else "") + value
    try:
        yield
    finally:
        if saved is None:
            del os.environ["ISOCON_DEBUG_VARIANT"]
        else:
            os.environ["ISOCON_DEBUG_VARIANT"] = saved


def raw_call(st, q, t, k, cap):
    """isocon_hw_locations_wide itself: (status, ed, loc_ptr, locs, needed)"""
    from isocon_amd import _lib
    from isocon_amd.store import _ptr
    q, t, k = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.int32)
    n = len(q)
    ed = np.full(n, -77, dtype=np.int32)
    ptr = np.full(n + 1, 2 ** 60, dtype=np.uint64)
    locs = np.full((max(cap, 1), 2), -77, dtype=np.int32)
    needed, ms = ctypes.c_uint64(2 ** 60), ctypes.c_float(-1)
    rc = st._L.isocon_hw_locations_wide(st._h, _ptr(q, _lib.u32p), _ptr(t, _lib.u32p), _ptr(k, _lib.i32p), n, _ptr(ed, _lib.i32p), _ptr(ptr, _lib.u64p),
                                        _ptr(locs, _lib.i32p), cap, ctypes.byref(needed), ctypes.byref(ms))
    return rc, ed, ptr, locs, int(needed.value)


def unpack(ed, ptr, locs):
    return [(int(ed[p]), tuple((int(s), int(e)) for s, e in locs[int(ptr[p]):int(ptr[p + 1])].tolist())) for p in range(len(ed))]


def compare(got, exp, names):
    bad = [(nm, g[0], g[1][:3], e[0], e[1][:3]) for g, e, nm in zip(got, exp, names) if g != (e[0], tuple(e[1]))]
    assert not bad, (len(bad), len(got), bad[:5])


def check_against_hw_pairs(got, rows):
    for g, r in zip(got, rows.tolist()):
        assert g[0] == r[0] and (g[1][0] == (r[1], r[2]) if r[0] >= 0 else g[1] == ()), (g[0], g[1][:2], r)


def run_list(seqs, q, t, k):
    """(got, stats) of one wide call on a store of seqs, the first locations checked against hw_pairs(wide=True)"""
    from isocon_amd.store import SeqStore
    st = SeqStore(list(seqs))
    try:
        ed, ptr, locs = st.hw_locations(q, t, k, wide=True)
        stats = st.hw_locations_wide_last_stats()
        rows = np.asarray(st.hw_pairs(q, t, k, wide=True)).copy()
    finally:
        st.close()
    assert ptr[0] == 0 and len(locs) == ptr[-1] and (np.diff(ptr.astype(np.int64)) >= 0).all()
    got = unpack(ed, ptr, locs)
    check_against_hw_pairs(got, rows)
    return got, stats


def run_cases(case_list, exp, rows_max=W.ROWS_MAX):
    """the cases in one call: every pair equals the restatement and the stats show the routes claimed"""
    seqs, q, t, k = W.flatten(case_list)
    got, stats = run_list(seqs, q, t, k)
    compare(got, exp, [c.name for c in case_list])
    routes = [W.route_of(len(c.query), len(c.target), c.k, rows_max) for c in case_list]
    for route, key in ROUTE_KEYS.items():
        assert stats[key] == routes.count(route), (key, stats)
    wide = sum(r in ROUTE_KEYS for r in routes)
    assert stats["pairs"] == len(case_list) and stats["wide"] == wide and stats["narrow"] + stats["wide"] == stats["pairs"], stats
    assert stats["hits"] == sum(e[0] >= 0 for e in exp) and stats["locations"] == sum(len(e[1]) for e in exp), stats
    assert (stats["launches"] > 0) == (wide > 0), stats
    return got, stats


# ---- word and route edges -------------------------------------------------------------------------------------------------------------
def test_word_and_route_edges():
    got, stats = run_cases(W.cases("edges"), W.expected("edges"))
    assert stats["rows_w1"] == 4 * 7 and stats["rows_w2"] == 3 * 7 and stats["rows_w4"] == 3 * 7 and stats["wave"] == 4 and stats["narrow"] == 0


def test_queries_of_65_to_256_rows_on_the_wavefront_route():
    cs = [c for c in W.cases("edges") if 65 <= len(c.query) <= 256]
    exp = [e for c, e in zip(W.cases("edges"), W.expected("edges")) if 65 <= len(c.query) <= 256]
    with variant("hwl_rows_max=64"):
        got, stats = run_cases(cs, exp, rows_max=64)
    assert stats["wave"] == len(cs) == 6 * 7 and stats["rows_w2"] == stats["rows_w4"] == 0


def test_queries_of_129_to_256_rows_on_either_side_of_a_switch_at_128():
    cs = [c for c in W.cases("edges") if len(c.query) <= 256]
    exp = [e for c, e in zip(W.cases("edges"), W.expected("edges")) if len(c.query) <= 256]
    with variant("hwl_rows_max=128"):
        got, stats = run_cases(cs, exp, rows_max=128)
    assert stats["rows_w2"] == 3 * 7 and stats["rows_w4"] == 0 and stats["wave"] == 3 * 7


# ---- where copies sit, thresholds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ("copies", "thresholds"))
def test_group_equals_restatement(group):
    got, stats = run_cases(W.cases(group), W.expected(group))
    by = dict(zip((c.name for c in W.cases(group)), got))
    if group == "copies":
        assert by["copies_first_column"][1][0][0] == 0 and by["copies_better_after_worse"][0] == 0 and len(by["copies_better_after_worse"][1]) == 1
        assert len(by["copies_equal_around_worse"][1]) == 2 and len(by["copies_overlap"][1]) == 2
        assert stats["starts_banded"] == stats["locations"] and stats["starts_unbanded"] == 0
    else:
        assert by["thr_k_below"] == (-1, ()) and by["thr_k_equal"][0] == 3 and by["thr_short_by_k"][0] == 300 and by["thr_short_by_k_plus_1"] == (-1, ())
        assert by["thr_empty_query"] == by["thr_empty_target"] == (-1, ())
        assert stats["starts_unbanded"] == len(by["thr_short_by_k"][1]) >= 1          # h = 300: beyond the banded START


# ---- every column an end ------------------------------------------------------------------------------------------------------------
def test_every_column_an_end():
    c20, c300 = W.cases("all")
    e20, e300 = W.expected("all")
    got, stats = run_cases([c20], [e20])
    assert got[0][0] == 20 and len(got[0][1]) == 700 and stats["rows_w1"] == 1 and stats["starts_banded"] == 700 and stats["starts_unbanded"] == 0
    got, stats = run_cases([c300], [e300])
    assert got[0][0] == 300 and len(got[0][1]) == 310 and stats["wave"] == 1 and stats["starts_unbanded"] == 310 and stats["starts_banded"] == 0
    got, stats = run_cases([c20, c300], [e20, e300])
    assert stats["starts_banded"] == 700 and stats["starts_unbanded"] == 310


# ---- lanes of one wave that finish apart -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", W.LIST_SIZES)
def test_lanes_of_one_wave_finish_apart(size):
    pick = [i for i, c in enumerate(W.cases("lanes")) if c.name.startswith("lanes%d_" % size)]
    cs, exp = [W.cases("lanes")[i] for i in pick], [W.expected("lanes")[i] for i in pick]
    got, stats = run_cases(cs, exp)
    assert stats["rows_w1"] == size and [len(g[1]) for g in got] == [c.n_ends for c in cs]
    assert 600 <= min(len(c.target) for c in cs) and max(len(c.target) for c in cs) <= 1500


# ---- narrow and wide pairs interleaved ---------------------------------------------------------------------------------------------
def test_mixed_list():
    from isocon_amd.store import SeqStore
    cs, exp = W.cases("mixed"), W.expected("mixed")
    got, stats = run_cases(cs, exp)
    assert stats["narrow"] == 4 and stats["wide"] == 4
    seqs, q, t, k = W.flatten(cs)
    assert q[2] == q[4] and t[2] == t[4] and k[2] != k[4] and got[2] == got[4]          # the same pair on both routes
    narrow = [i for i, c in enumerate(cs) if c.route in ("narrow", "none")]
    st = SeqStore(seqs)
    try:
        # the narrow rows are those of a plain call on them; a list with no wide pair launches nothing of the wide part
        ed, ptr, locs = st.hw_locations([q[i] for i in narrow], [t[i] for i in narrow], [k[i] for i in narrow])
        assert unpack(ed, ptr, locs) == [got[i] for i in narrow]
        ed2, ptr2, locs2 = st.hw_locations([q[i] for i in narrow], [t[i] for i in narrow], [k[i] for i in narrow], wide=True)
        stats = st.hw_locations_wide_last_stats()
        assert unpack(ed2, ptr2, locs2) == [got[i] for i in narrow]
        assert stats["launches"] == 0 and stats["wide"] == 0 and stats["narrow"] == stats["pairs"] == len(narrow) and stats["locations"] == len(locs2)
    finally:
        st.close()


# ---- the random list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_max", (W.ROWS_MAX, 64))
def test_random_list_equals_restatement(rows_max):
    seqs, q, t, k = W.random_list()
    exp = [W.L.restated_cached(seqs[a], seqs[b], kk) for a, b, kk in zip(q, t, k)]
    with variant("hwl_rows_max=%d" % rows_max):
        got, stats = run_list(seqs, q, t, k)
    compare(got, exp, list(range(len(q))))
    routes = [W.route_of(len(seqs[a]), len(seqs[b]), kk, rows_max) for a, b, kk in zip(q, t, k)]
    for route, key in ROUTE_KEYS.items():
        assert stats[key] == routes.count(route), (key, stats)
    assert stats["narrow"] == routes.count("narrow") + routes.count("none") > 0 and stats["starts_banded"] > 0
    assert stats["starts_banded"] + stats["starts_unbanded"] == sum(len(e[1]) for e, r in zip(exp, routes) if r in ROUTE_KEYS)


# ---- capacity and arguments ----------------------------------------------------------------------------------------------------------
def test_capacity_protocol_and_arguments():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    cs, exp = W.cases("mixed"), W.expected("mixed")
    seqs, q, t, k = W.flatten(cs)
    names = [c.name for c in cs]
    total = sum(len(e[1]) for e in exp)
    st = SeqStore(seqs)
    try:
        rc, ed, ptr, locs, needed = raw_call(st, q, t, k, 0)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == total > 0
        assert ed.tolist() == [e[0] for e in exp] and ptr.tolist() == np.concatenate([[0], np.cumsum([len(e[1]) for e in exp])]).tolist()
        rc, ed, ptr, locs, needed = raw_call(st, q, t, k, total - 1)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == total and (locs == -77).all()
        rc, ed, ptr, locs, needed = raw_call(st, q, t, k, total)
        assert rc == _lib.ISOCON_OK and needed == total
        compare(unpack(ed, ptr, locs), exp, names)
        # wide pairs alone
        wide = [i for i, c in enumerate(cs) if c.route not in ("narrow", "none")]
        wq, wt, wk = [q[i] for i in wide], [t[i] for i in wide], [k[i] for i in wide]
        wtotal = sum(len(exp[i][1]) for i in wide)
        rc, ed, ptr, locs, needed = raw_call(st, wq, wt, wk, wtotal - 1)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == wtotal and (locs == -77).all() and ed.tolist() == [exp[i][0] for i in wide]
        rc, ed, ptr, locs, needed = raw_call(st, wq, wt, wk, wtotal)
        assert rc == _lib.ISOCON_OK
        compare(unpack(ed, ptr, locs), [exp[i] for i in wide], [names[i] for i in wide])
        # no pairs
        rc, ed, ptr, locs, needed = raw_call(st, [], [], [], 0)
        assert rc == _lib.ISOCON_OK and ptr.tolist() == [0] and needed == 0
        ed, ptr, locs = st.hw_locations([], [], None, wide=True)
        assert len(ed) == 0 and ptr.tolist() == [0] and locs.shape == (0, 2)
        # an id out of range, a negative threshold, one above 2^20
        assert raw_call(st, [len(seqs)], [0], [1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_call(st, [q[1]], [t[1]], [-1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_call(st, [q[1]], [t[1]], [2 ** 20 + 1], 8)[0] == _lib.ISOCON_E_UNSUPPORTED
        assert raw_call(st, [q[1]], [t[1]], [2 ** 20], 8)[0] == _lib.ISOCON_OK
        # the banded entry keeps refusing the wide pair
        with pytest.raises(_lib.IsoconError) as err:
            st.hw_locations([q[1]], [t[1]], [k[1]], wide=False)
        assert err.value.status == _lib.ISOCON_E_UNSUPPORTED
    finally:
        st.close()


def test_alphabets():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    c = W.cases("copies")[8]          # two copies, one substitution each
    exp = W.expected("copies")[8]
    st = SeqStore([c.query, c.target, "ACGTN"])
    try:
        rc = raw_call(st, [0], [1], [c.k], 16)[0]
        assert rc == _lib.ISOCON_E_ALPHABET
    finally:
        st.close()
    st = SeqStore([c.query.lower(), c.target.lower()])
    try:
        ed, ptr, locs = st.hw_locations([0], [1], [c.k], wide=True)
        compare(unpack(ed, ptr, locs), [exp], [c.name])
        assert st.hw_locations_wide_last_stats()["rows_w1"] == 1
    finally:
        st.close()


def test_two_pass_query_against_a_target_beyond_the_boundary_buffer_is_refused_before_any_launch():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    st = SeqStore(["ACG" * 1365 + "AC", "T" * 655361, "ACGACGACGTACGTTACGATCGATCGGCTA"])
    try:
        assert st.lens[0] == 4097
        rc = raw_call(st, [2, 0], [1, 1], [2, 4097], 16)[0]
        stats = st.hw_locations_wide_last_stats()
        assert rc == _lib.ISOCON_E_UNSUPPORTED and stats["launches"] == 0 and stats["wide"] == 2
    finally:
        st.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_python_entry():
    import random
    from isocon_amd import edlib_alignment_module as EAM
    rng = random.Random("test_gpu_hw_locations_wide/python")
    primer = W.body(rng, 30)
    one = W.plant(primer, 1, "sub")
    read, ends = W.spaced([one, one, one], [400, 700, 900], 2500 - 2000 - 3 * 30)
    assert len(read) == 2500
    want = [(e - 29, e) for e in ends]
    assert W.restated(primer, read, 2) == (1, want)
    before = EAM.TRACEBACK_INFIX_ALL_STATS["device"]
    ed, locs, cigar = EAM.edlib_traceback_infix_all(primer, read, k=2)
    assert (ed, locs) == (1, want)
    assert cigar == EAM.edlib_traceback_infix(primer, read, k=2)[2] and sum(int(x) for x in cigar.replace("X", "=").split("=") if x) == 30
    assert EAM.edlib_traceback_infix_all(primer, read, k=None)[:2] == (1, want)
    assert EAM.edlib_traceback_infix_all(primer, read, k=0) == (-1, [], None)
    # a query of 300 bases with k=None: sent as k = 300, a band of 601 diagonals and more
    c = W.cases("edges")[-3]
    assert len(c.query) == 300
    h, want300 = W.expected("edges")[-3]
    ed, locs, cigar = EAM.edlib_traceback_infix_all(c.query, c.target, k=None)
    assert (ed, locs) == (h, list(want300)) and cigar == EAM.edlib_traceback_infix(c.query, c.target, k=None)[2]
    assert EAM.TRACEBACK_INFIX_ALL_STATS["device"] == before + 4
