"""GPU: isocon_hw_locations (csrc/hw_loc.hpp, hw_loc_host.inc) -- every best location of an infix pair -- on the designed inputs of
tests/hw_locations_cases.py and on a random list, through the C ABI: distance, row pointers and every (start, end) of EVERY pair
against the plain restatement, the first location against isocon_hw_pairs, the call's protocol (capacity, empty list, alphabet, band
limit) and the Python entry.  tests/test_hw_locations_cases.py shows on the CPU that the inputs sit where they claim to."""
import ctypes

import numpy as np
import pytest

import hw_locations_cases as C

pytestmark = pytest.mark.gpu


def raw_call(st, q, t, k, cap):
    """isocon_hw_locations itself: (status, ed, loc_ptr, locs, needed)"""
    from isocon_amd import _lib
    from isocon_amd.store import _ptr
    q, t, k = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.int32)
    n = len(q)
    ed = np.full(n, -77, dtype=np.int32)
    ptr = np.full(n + 1, 2 ** 60, dtype=np.uint64)
    locs = np.full((max(cap, 1), 2), -77, dtype=np.int32)
    needed, ms = ctypes.c_uint64(2 ** 60), ctypes.c_float(-1)
    rc = st._L.isocon_hw_locations(st._h, _ptr(q, _lib.u32p), _ptr(t, _lib.u32p), _ptr(k, _lib.i32p), n, _ptr(ed, _lib.i32p), _ptr(ptr, _lib.u64p),
                                   _ptr(locs, _lib.i32p), cap, ctypes.byref(needed), ctypes.byref(ms))
    return rc, ed, ptr, locs, int(needed.value)


def unpack(ed, ptr, locs):
    return [(int(ed[p]), tuple((int(s), int(e)) for s, e in locs[int(ptr[p]):int(ptr[p + 1])].tolist())) for p in range(len(ed))]


def compare(got, exp, names):
    bad = [(nm, g[0], g[1][:3], e[0], e[1][:3]) for g, e, nm in zip(got, exp, names) if g != e]
    assert not bad, (len(bad), len(got), bad[:5])


def run_cases(case_list, group):
    """(got, exp, names, hw_pairs rows, stats) of one call on a store of the cases"""
    from isocon_amd.store import SeqStore, hw_locations_last_stats
    seqs, q, t, k, owner = C.flatten(case_list)
    exp = [C.expected(group)[c.name, lane] for c, lane in owner]
    st = SeqStore(seqs)
    try:
        ed, ptr, locs = st.hw_locations(q, t, k)
        stats = hw_locations_last_stats()
        rows = np.asarray(st.hw_pairs(q, t, k)).copy()
    finally:
        st.close()
    assert ptr[0] == 0 and len(locs) == ptr[-1] and (np.diff(ptr.astype(np.int64)) >= 0).all()
    return unpack(ed, ptr, locs), exp, [(c.name, lane) for c, lane in owner], rows, stats


def check_against_hw_pairs(got, rows):
    for g, r in zip(got, rows.tolist()):
        assert g[0] == r[0] and (g[1][0] == (r[1], r[2]) if r[0] >= 0 else g[1] == ()), (g[0], g[1][:2], r)


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_group_equals_restatement(group):
    got, exp, names, rows, stats = run_cases(C.cases(group), group)
    compare(got, exp, names)
    check_against_hw_pairs(got, rows)
    assert stats["pairs"] == len(got) and stats["hits"] == sum(e[0] >= 0 for e in exp) and stats["locations"] == sum(len(e[1]) for e in exp)
    ends_w = {w for w in (1, 2, 4, 8) if stats["ends_tiles_w%d" % w]}
    starts_w = {w for w in (1, 2, 4, 8) if stats["starts_tiles_w%d" % w]}
    if group == "a":
        # (a_wide_b_k63: LOCATE bands of 505 and 512 diagonals on one query, 568 in common -- that stage's tiles are cut on the host)
        assert ends_w == starts_w == {1, 2, 4, 8} and stats["host_cuts"] == 1
    elif group == "e":
        assert stats["host_cuts"] == 2 and stats["locate_tiles_w8"] == stats["ends_tiles_w8"] == 2          # LOCATE and ENDS, a tile per pair
    else:
        assert stats["host_cuts"] == 0


def test_one_and_forty_ends_in_one_tile_and_a_pair_over_two_start_tiles():
    c, = [c for c in C.cases("d") if c.name == "d_1_and_40"]
    got, exp, names, rows, stats = run_cases([c], "d")
    compare(got, exp, names)
    assert [len(g[1]) for g in got] == [40, 1, 30]
    assert stats["ends_tiles_w8"] == 1 and sum(stats["ends_tiles_w%d" % w] for w in (1, 2, 4)) == 0
    assert stats["starts_tiles_w1"] == 2 and stats["locations"] == 71          # 64 + 7 entries: no subset of 40, 1, 30 makes 7


@pytest.mark.parametrize("n", C.TILE_SIZES)
def test_many_targets_on_one_query(n):
    c, = [c for c in C.cases("d") if c.name == "d_targets%d" % n]
    got, exp, names, rows, stats = run_cases([c], "d")
    compare(got, exp, names)
    assert stats["hits"] == n and stats["ends_tiles_w1"] == (n + 63) // 64 and stats["starts_tiles_w1"] == (stats["locations"] + 63) // 64


def test_capacity_protocol():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    seqs, q, t, k, owner = C.flatten(C.cases("c"))
    exp = [C.expected("c")[c.name, lane] for c, lane in owner]
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
        compare(unpack(ed, ptr, locs), exp, [(c.name, lane) for c, lane in owner])
        # no pairs
        rc, ed, ptr, locs, needed = raw_call(st, [], [], [], 0)
        assert rc == _lib.ISOCON_OK and ptr.tolist() == [0] and needed == 0
        ed, ptr, locs = st.hw_locations([], [], None)
        assert len(ed) == 0 and ptr.tolist() == [0] and locs.shape == (0, 2)
        # arguments as isocon_hw_pairs: an id out of range, a negative threshold
        assert raw_call(st, [len(seqs)], [0], [1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_call(st, [0], [1], [-1], 8)[0] == _lib.ISOCON_E_ARG
    finally:
        st.close()


def test_alphabet_and_band_limit():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    c, = [c for c in C.cases("c") if c.name == "c_exact_x5"]
    exp = C.expected("c")[c.name, 0]
    st = SeqStore([c.query, c.targets[0], "ACGTN"])
    try:
        with pytest.raises(_lib.IsoconError) as err:
            st.hw_locations([0], [1], [0])
        assert err.value.status == _lib.ISOCON_E_ALPHABET
    finally:
        st.close()
    st = SeqStore([c.query.lower(), c.targets[0].lower()])          # its own four-symbol map
    try:
        ed, ptr, locs = st.hw_locations([0], [1], 3)
        assert unpack(ed, ptr, locs) == [exp] and len(exp[1]) == 5
        # k None / negative: unbounded, sent as len(q)
        assert unpack(*st.hw_locations([0, 0], [1, 1], [-1, 0])) == [exp, exp]
        assert unpack(*st.hw_locations([0], [1], None)) == [exp]
    finally:
        st.close()
    q = C.body(C._rng("limit"), 300)
    st = SeqStore([q, q + "T" * 40, "T" * 300 + q])
    try:
        with pytest.raises(_lib.IsoconError) as err:          # 40 + 2 x 236 + 1 = 513 diagonals
            st.hw_locations([0, 0], [1, 1], [3, 236])
        assert err.value.status == _lib.ISOCON_E_UNSUPPORTED
        with pytest.raises(_lib.IsoconError) as err:          # 300 + 2 x 106 + 1 = 513
            st.hw_locations([0], [2], [106])
        assert err.value.status == _lib.ISOCON_E_UNSUPPORTED
        assert unpack(*st.hw_locations([0, 0], [1, 2], [235, 105])) == [(0, ((0, 299),)), (0, ((300, 599),))]          # 511 and 511 (together: cut on the host)
    finally:
        st.close()


def test_random_list_consistent_with_hw_pairs_and_restatement():
    from isocon_amd.store import SeqStore
    seqs, q, t, k = C.random_list()
    exp = [C.restated_cached(seqs[a], seqs[b], kk) for a, b, kk in zip(q, t, k)]
    st = SeqStore(list(seqs))
    try:
        ed, ptr, locs = st.hw_locations(q, t, k)
        rows = np.asarray(st.hw_pairs(q, t, k)).copy()
    finally:
        st.close()
    got = unpack(ed, ptr, locs)
    assert (ed == rows[:, 0]).all()
    check_against_hw_pairs(got, rows)
    compare(got, exp, list(range(len(q))))


def test_python_entry_all_locations():
    from isocon_amd import edlib_alignment_module as EAM
    rng = C._rng("python")
    x = C.body(rng, 25)
    copy = C.plant(x, 1, "sub")
    y, ends = C.spaced([copy] * 3, [9, 30, 12], 6)
    before = dict(EAM.TRACEBACK_INFIX_ALL_STATS), dict(EAM.TRACEBACK_INFIX_STATS)
    ed, locations, cigar = EAM.edlib_traceback_infix_all(x, y, k=2)
    assert (ed, locations) == (1, [(e - 24, e) for e in ends]) and C.restated(x, y, 2) == (ed, locations)
    one = EAM.edlib_traceback_infix(x, y, k=2)
    assert one == (ed, locations[:1], cigar) and cigar.count("X") == 1 and sum(int(n) for n in cigar.replace("X", "=").split("=") if n) == 25
    assert EAM.edlib_traceback_infix_all(x, y, k=0) == (-1, [], None)
    assert EAM.edlib_traceback_infix_all(x, "", k=3) == (-1, [], None) and EAM.edlib_traceback_infix_all("", y, k=3) == (-1, [], None)
    assert EAM.edlib_traceback_infix_all(x, y, k=None)[:2] == (ed, locations)
    assert EAM.TRACEBACK_INFIX_ALL_STATS["device"] == before[0]["device"] + 5 and EAM.TRACEBACK_INFIX_STATS["device"] == before[1]["device"] + 1
