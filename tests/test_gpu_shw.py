"""GPU: the prefix ("SHW") entries isocon_shw_locations and isocon_shw_path_pairs (csrc/shw.hpp, shw_host.inc) on the designed inputs of
tests/shw_cases.py and on a random list, through the C ABI: distance, row pointers and every end of EVERY pair against the plain
restatement, every end again against the oracle's global distance, the paths against oracle.nw_path, the rounds and tiles the call
reports, the call's protocol and the Python entry.  tests/test_shw_cases.py shows on the CPU that the inputs sit where they claim to."""
import ctypes
import os

import numpy as np
import pytest

import shw_cases as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def raw_locations(st, q, t, k, cap):
    """isocon_shw_locations itself: (status, ed, end_ptr, ends, needed)"""
    from isocon_amd import _lib
    from isocon_amd.store import _ptr
    q, t, k = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.int32)
    n = len(q)
    ed = np.full(n, -77, dtype=np.int32)
    ptr = np.full(n + 1, 2 ** 60, dtype=np.uint64)
    ends = np.full(max(cap, 1), -77, dtype=np.int32)
    needed, ms = ctypes.c_uint64(2 ** 60), ctypes.c_float(-1)
    rc = st._L.isocon_shw_locations(st._h, _ptr(q, _lib.u32p), _ptr(t, _lib.u32p), _ptr(k, _lib.i32p), n, _ptr(ed, _lib.i32p), _ptr(ptr, _lib.u64p),
                                    _ptr(ends, _lib.i32p), cap, ctypes.byref(needed), ctypes.byref(ms))
    return rc, ed, ptr, ends, int(needed.value)


def raw_paths(st, q, t, k, cap):
    """isocon_shw_path_pairs itself: (status, rows, ops_ptr, ops, needed)"""
    from isocon_amd import _lib
    from isocon_amd.store import _ptr
    q, t, k = np.ascontiguousarray(q, dtype=np.uint32), np.ascontiguousarray(t, dtype=np.uint32), np.ascontiguousarray(k, dtype=np.int32)
    n = len(q)
    rows = np.full((n, 2), -77, dtype=np.int32)
    ptr = np.full(n + 1, 2 ** 60, dtype=np.uint64)
    ops = np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32)
    needed, ms = ctypes.c_uint64(2 ** 60), ctypes.c_float(-1)
    rc = st._L.isocon_shw_path_pairs(st._h, _ptr(q, _lib.u32p), _ptr(t, _lib.u32p), _ptr(k, _lib.i32p), n, _ptr(rows, _lib.i32p), _ptr(ops, _lib.u32p),
                                     _ptr(ptr, _lib.u64p), cap, ctypes.byref(needed), ctypes.byref(ms))
    return rc, rows, ptr, ops, int(needed.value)


def unpack(ed, ptr, ends):
    return [(int(ed[p]), tuple(ends[int(ptr[p]):int(ptr[p + 1])].tolist())) for p in range(len(ed))]


def compare(got, exp, names):
    bad = [(nm, g[0], g[1][:3], e[0], e[1][:3]) for g, e, nm in zip(got, exp, names) if g != e]
    assert not bad, (len(bad), len(got), bad[:5])


def expected_stats(seqs, q, t, k):
    """what isocon_shw_last_stats must report for the list, from the driver's rules restated in tests/shw_cases.py and the restatement"""
    n = len(q)
    P = [len(seqs[a]) for a in q]
    N = [len(seqs[b]) for b in t]
    hu = [C.restated_cached(seqs[a], seqs[b], None)[0] for a, b in zip(q, t)]
    kc = [C.clamp(kk, p) for kk, p in zip(k, P)]
    out = {"pairs": n, "rounds": 0}
    for w in (1, 2, 4, 8):
        out["locate_tiles_w%d" % w] = out["ends_tiles_w%d" % w] = 0
    for r in range(4):
        out["enter_round%d" % r] = 0

    def tiles(thr, take, key):
        count = {}
        for p in range(n):
            if take[p]:
                count[q[p], C.words(2 * thr[p] + 1)] = count.get((q[p], C.words(2 * thr[p] + 1)), 0) + 1
        for (_, w), c in count.items():
            out[key % w] += (c + 63) // 64

    open_ = [True] * n
    hit = [False] * n
    for r, cap in enumerate(C.ROUND_THR):
        if r and not any(open_):
            break
        out["rounds"] = r + 1
        out["enter_round%d" % r] = sum(open_)
        thr = [min(x, cap) for x in kc]
        need = [open_[p] and C.needs_kernel(P[p], N[p], thr[p]) for p in range(n)]
        tiles(thr, need, "locate_tiles_w%d")
        for p in range(n):
            if open_[p]:
                hit[p] = need[p] and 0 <= hu[p] <= thr[p]
                open_[p] = not (hit[p] or thr[p] == kc[p])
    out["hits"] = sum(hit)
    tiles(hu, hit, "ends_tiles_w%d")
    return out, any(open_)


def encode(path):
    return [(n << 4) | "=XID".index(op) for n, op in path]


def check_path(x, y_prefix, h, ops):
    """what holds for every path, whatever the oracle says: it spells both strings and costs h"""
    i = j = cost = 0
    for o in ops:
        n, op = o >> 4, "=XID"[o & 15]
        assert n > 0
        if op in "=X":
            assert all((x[i + s] == y_prefix[j + s]) == (op == "=") for s in range(n))
            i += n; j += n
        elif op == "I":
            i += n
        else:
            j += n
        cost += n if op != "=" else 0
    assert (i, j, cost) == (len(x), len(y_prefix), h)


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_group_equals_restatement_oracle_and_paths(group):
    from isocon_amd.store import SeqStore, shw_last_stats
    seqs, q, t, k, owner = C.flatten(C.cases(group))
    exp = [C.expected(group)[c.name, lane] for c, lane in owner]
    names = [(c.name, lane) for c, lane in owner]
    want, refused = expected_stats(seqs, q, t, k)
    assert not refused
    st = SeqStore(seqs)
    try:
        ed, ptr, ends = st.shw_locations(q, t, C.send_k(k))
        stats = shw_last_stats()
        rows, ops, ops_ptr = st.shw_path_pairs(q, t, C.send_k(k))
        stats_path = shw_last_stats()
    finally:
        st.close()
    assert ptr[0] == 0 and len(ends) == ptr[-1] and (np.diff(ptr.astype(np.int64)) >= 0).all()
    got = unpack(ed, ptr, ends)
    compare(got, exp, names)
    # second opinion: every reported end against the oracle's global distance
    for (h, ee), a, b in zip(got, q, t):
        for e in ee:
            assert O.ed_dp(seqs[a], seqs[b][:e + 1]) == h, (a, b, e, h)
    # the call's own account of itself
    want["ends"] = sum(len(e[1]) for e in exp)
    assert stats == want, (stats, want)
    assert {key: v for key, v in stats_path.items() if not key.startswith("ends")} == {key: v for key, v in want.items() if not key.startswith("ends")}
    # paths: the rows, then the ops of the first end against the oracle
    assert rows[:, 0].tolist() == [e[0] for e in exp] and rows[:, 1].tolist() == [e[1][0] if e[0] >= 0 else -1 for e in exp]
    assert ops_ptr[0] == 0 and ops_ptr[-1] == len(ops)
    for p, (h, ee) in enumerate(exp):
        mine = ops[int(ops_ptr[p]):int(ops_ptr[p + 1])].tolist()
        if h < 0:
            assert mine == []
            continue
        x, y = seqs[q[p]], seqs[t[p]][:ee[0] + 1]
        d, path = O.nw_path(x, y)
        assert d == h and mine == encode(path), (names[p], h, mine[:4], path[:4])
        check_path(x, y, h, mine)


def test_rounds_of_group_e_and_the_refused_pair():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore, shw_last_stats
    c, = C.cases("e")
    seqs, q, t, k, owner = C.flatten([c])
    query, far = C.far_pair()
    assert query == seqs[0]
    st = SeqStore(seqs + [far])
    try:
        ed, ptr, ends = st.shw_locations(q, t, None)
        stats = shw_last_stats()
        assert ed.tolist() == [l["h"] for l in c.lanes]
        assert stats["rounds"] == 4 and [stats["enter_round%d" % r] for r in range(4)] == [8, 6, 4, 2]
        assert [stats["locate_tiles_w%d" % w] for w in (1, 2, 4, 8)] == [1, 1, 1, 1] == [stats["ends_tiles_w%d" % w] for w in (1, 2, 4, 8)]
        # the same list plus the far pair, in the middle: refused, and the message names it
        q2, t2 = q[:3] + [0] + q[3:], t[:3] + [len(seqs)] + t[3:]
        for call in (st.shw_locations, st.shw_path_pairs):
            with pytest.raises(_lib.IsoconError) as err:
                call(q2, t2, None)
            assert err.value.status == _lib.ISOCON_E_UNSUPPORTED and "pair 3 " in str(err.value), str(err.value)
        # under a threshold of 255 it is a plain miss
        ed, ptr, ends = st.shw_locations(q2, t2, 255)
        assert ed.tolist() == [l["h"] for l in c.lanes[:3]] + [-1] + [l["h"] for l in c.lanes[3:]]
    finally:
        st.close()


def test_unbounded_list_of_small_distances_runs_one_word_tiles_only():
    from isocon_amd.store import SeqStore, shw_last_stats
    case_list = [c for c in C.cases("d") if c.name.startswith("d_targets")]
    seqs, q, t, k, owner = C.flatten(case_list)
    exp = [C.restated_cached(seqs[a], seqs[b], None) for a, b in zip(q, t)]
    assert max(e[0] for e in exp) <= 31 and max(len(seqs[a]) for a in q) > 31
    st = SeqStore(seqs)
    try:
        got = unpack(*st.shw_locations(q, t, None))
        stats = shw_last_stats()
    finally:
        st.close()
    compare(got, exp, list(range(len(q))))
    assert stats["rounds"] == 1 and stats["hits"] == len(q) == stats["enter_round0"]
    assert stats["locate_tiles_w1"] == stats["ends_tiles_w1"] == sum((n + 63) // 64 for n in C.TILE_SIZES)
    assert sum(stats["%s_tiles_w%d" % (s, w)] for s in ("locate", "ends") for w in (2, 4, 8)) == 0


def test_protocol():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    seqs, q, t, k, owner = C.flatten(C.cases("c"))
    kk = C.send_k([C.clamp(x, len(seqs[a])) for x, a in zip(k, q)])
    exp = [C.expected("c")[c.name, lane] for c, lane in owner]
    names = [(c.name, lane) for c, lane in owner]
    total = sum(len(e[1]) for e in exp)
    st = SeqStore(seqs + [""])
    try:
        # capacity too small: the distances and pointers are valid, the ends untouched
        rc, ed, ptr, ends, needed = raw_locations(st, q, t, kk, 0)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == total > 0
        assert ed.tolist() == [e[0] for e in exp] and ptr.tolist() == np.concatenate([[0], np.cumsum([len(e[1]) for e in exp])]).tolist()
        rc, ed, ptr, ends, needed = raw_locations(st, q, t, kk, total - 1)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == total and (ends == -77).all()
        rc, ed, ptr, ends, needed = raw_locations(st, q, t, kk, total)
        assert rc == _lib.ISOCON_OK and needed == total
        compare(unpack(ed, ptr, ends), exp, names)
        rc, rows, optr, ops, needed = raw_paths(st, q, t, kk, 0)
        assert rc == _lib.ISOCON_E_CAPACITY and needed > 0 and rows[:, 0].tolist() == [e[0] for e in exp] and optr[-1] == needed
        rc, rows, optr, ops, needed2 = raw_paths(st, q, t, kk, needed)
        assert rc == _lib.ISOCON_OK and needed2 == needed and rows[:, 1].tolist() == [e[1][0] if e[0] >= 0 else -1 for e in exp]
        # an empty list
        rc, ed, ptr, ends, needed = raw_locations(st, [], [], [], 0)
        assert rc == _lib.ISOCON_OK and ptr.tolist() == [0] and needed == 0
        rc, rows, optr, ops, needed = raw_paths(st, [], [], [], 0)
        assert rc == _lib.ISOCON_OK and optr.tolist() == [0] and needed == 0
        ed, ptr, ends = st.shw_locations([], [], None)
        assert len(ed) == 0 and ptr.tolist() == [0] and ends.shape == (0,)
        # an empty sequence on either side: a miss
        empty = len(seqs)
        got = unpack(*st.shw_locations([empty, 0, empty], [1, empty, empty], [5, 5, -1]))
        assert got == [(-1, ()), (-1, ()), (-1, ())]
        assert st.shw_path_pairs([empty, 0], [1, empty], 5)[0].tolist() == [[-1, -1], [-1, -1]]
        # k < 0 and an id out of range, on either side
        assert raw_locations(st, [0], [1], [-1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_paths(st, [0], [1], [-3], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_locations(st, [0, 0], [1, 1], [2, -(1 << 30)], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_locations(st, [len(seqs) + 1], [0], [1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_locations(st, [0], [len(seqs) + 1], [1], 8)[0] == _lib.ISOCON_E_ARG
        assert raw_paths(st, [0, 0], [1, len(seqs) + 1], [1, 1], 8)[0] == _lib.ISOCON_E_ARG
        # (and the store still answers)
        assert unpack(*st.shw_locations(q[:3], t[:3], kk[:3])) == exp[:3]
    finally:
        st.close()
    # a fifth symbol
    st = SeqStore(["ACGT", "ACGTN"])
    try:
        for call in (st.shw_locations, st.shw_path_pairs):
            with pytest.raises(_lib.IsoconError) as err:
                call([0], [1], [1])
            assert err.value.status == _lib.ISOCON_E_ALPHABET
    finally:
        st.close()
    # a store under its own four-symbol map works unchanged
    st = SeqStore(["acgtc", "acgtac"])
    try:
        assert unpack(*st.shw_locations([0], [1], 2)) == [(1, (3, 4, 5))]
    finally:
        st.close()


def test_random_list_equals_restatement():
    from isocon_amd.store import SeqStore
    seqs, q, t, k = C.random_list()
    exp = [C.restated_cached(seqs[a], seqs[b], kk) for a, b, kk in zip(q, t, k)]
    st = SeqStore(list(seqs))
    try:
        got = unpack(*st.shw_locations(q, t, C.send_k(k)))
        rows, ops, ops_ptr = st.shw_path_pairs(q, t, C.send_k(k))
    finally:
        st.close()
    compare(got, exp, list(range(len(q))))
    assert rows[:, 0].tolist() == [e[0] for e in exp] and rows[:, 1].tolist() == [e[1][0] if e[0] >= 0 else -1 for e in exp]
    for p in range(0, len(q), 7):
        if exp[p][0] >= 0:
            check_path(seqs[q[p]], seqs[t[p]][:exp[p][1][0] + 1], exp[p][0], ops[int(ops_ptr[p]):int(ops_ptr[p + 1])].tolist())


def test_python_entry():
    from isocon_amd import edlib_alignment_module as EAM
    before = dict(EAM.TRACEBACK_PREFIX_STATS), dict(EAM.TRACEBACK_STATS)
    assert EAM.edlib_traceback_prefix("ACGTC", "ACGTAC", k=2) == (1, [(0, 3), (0, 4), (0, 5)], "4=1I")
    rng = C._rng("python")
    x = C.body(rng, 40)
    y = C.plant(x, 3, "sub") + C.rnd(rng, 500)
    h, ends = C.restated(x, y, None)
    d, path = O.nw_path(x, y[:ends[0] + 1])
    want = (h, [(0, e) for e in ends], "".join("%d%s" % o for o in path))
    assert h == d == 3 and EAM.edlib_traceback_prefix(x, y, k=None) == want == EAM.edlib_traceback_prefix(x, y, k=3) == EAM.edlib_traceback_prefix(x, y, k=-1)
    assert EAM.edlib_traceback_prefix(x, y, k=2) == (-1, [], None)          # a miss
    assert EAM.edlib_traceback_prefix(x, "", k=3) == (-1, [], None) and EAM.edlib_traceback_prefix("", y, k=3) == (-1, [], None)
    assert EAM.TRACEBACK_PREFIX_STATS["device"] == before[0]["device"] + 7 and EAM.TRACEBACK_STATS == before[1]
    for mode in ("SHW", "HW"):
        with pytest.raises(NotImplementedError):
            EAM.edlib_traceback(x, y, mode=mode)


def test_header_exports_and_ctypes_table_in_step():
    from isocon_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isocon_hip.h")).read()
    L = _lib.load()
    for name in ("isocon_shw_locations", "isocon_shw_path_pairs", "isocon_shw_last_stats"):
        assert "int %s(" % name in header and name in _lib.SYMBOLS and hasattr(L, name)
    assert len(_lib.SYMBOLS["isocon_shw_locations"][1]) == 11 == len(_lib.SYMBOLS["isocon_shw_path_pairs"][1])
