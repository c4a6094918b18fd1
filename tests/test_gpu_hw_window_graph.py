"""The candidate-vs-candidate graph with ignored ends built on the device (isocon_hw_window_graph, SeqStore.hw_window_graph): against the
reference's own outputs (tests/golden/g14_all_nn.json), the CPU oracle and the pair-list route that stays in the tree
(ISOCON_DEBUG_VARIANT=hw_host_graph); its refusals; and which route the product functions take."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hw_graph_cases as HC  # noqa: E402

G14 = json.load(open(os.path.join(HERE, "golden", "g14_all_nn.json")))
pytestmark = pytest.mark.gpu


def params_of(ignore_ends_len, depth):
    class Params(object):
        nr_cores = 1
        verbose = False
    Params.ignore_ends_len = ignore_ends_len
    Params.neighbor_search_depth = depth
    return Params()


def rows_of(g):
    return [(a, list(nb.items())) for a, nb in g.items()]


def both_forms(C, ignore_ends_len, depth):
    """(directed, symmetric) dicts from the device call, built by the product's own function"""
    from isocon_amd import end_invariant_functions as END
    lst = HC.sorted_list(C)
    directed = END._device_window_graph(lst, depth, ignore_ends_len, False)
    symmetric = END._device_window_graph(lst, depth, ignore_ends_len, True)
    assert directed is not None and symmetric is not None
    return lst, directed, symmetric


def counters_of(lst, ignore_ends_len, depth, symmetric):
    from isocon_amd.store import SeqStore
    st = SeqStore([s for s, _ in lst])
    try:
        return st.hw_window_graph(10 + 2 * ignore_ends_len, 10 + ignore_ends_len, depth, ignore_ends_len, 10, symmetric, return_counters=True)[3]
    finally:
        st.close()


# ---- the reference's outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G14["cases"], ids=[c["name"] for c in G14["cases"]])
def test_reference_fixtures(case):
    from oracle import oracle as O
    lst, directed, symmetric = both_forms(dict(case["C"]), case["ignore_ends_len"], case["neighbor_search_depth"])
    assert [[a, [list(x) for x in nb.items()]] for a, nb in symmetric.items()] == case["expect"]
    assert rows_of(directed) == rows_of(O.get_all_NN(lst, 0, 0, lst, case["neighbor_search_depth"], case["ignore_ends_len"]))


# ---- small families against the oracle -----------------------------------------------------------------------------------------
FAMILIES = {"five_cuts": HC.five_cuts, "family3": lambda: HC.family(3), "family4": lambda: HC.family(4)}


@pytest.mark.parametrize("depth", [1, 3, 2 ** 32])
@pytest.mark.parametrize("ignore_ends_len", [0, 5, 15])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_small_families_equal_oracle(name, ignore_ends_len, depth):
    from oracle import oracle as O
    C = FAMILIES[name]()
    lst, directed, symmetric = both_forms(C, ignore_ends_len, depth)
    assert rows_of(directed) == rows_of(O.get_all_NN(lst, 0, 0, lst, depth, ignore_ends_len))
    assert rows_of(symmetric) == rows_of(O.get_NN_graph_ignored_ends_edlib(C, params_of(ignore_ends_len, depth)))
    one_way = sum(1 for a, row in directed.items() for b in row if a not in directed[b])
    two_way = sum(1 for a, row in directed.items() for b in row if a in directed[b])
    ctr = counters_of(lst, ignore_ends_len, depth, True)
    assert ctr["directed"] == one_way + two_way and ctr["appended"] == one_way
    assert counters_of(lst, ignore_ends_len, depth, False)["appended"] == 0
    if ignore_ends_len == 15:
        # (checked with the oracle when the seeds were chosen: the cases cannot pass without an appended entry / a min of two directions)
        assert ctr["appended"] > 0 and one_way > 0 and two_way > 0
    if name == "five_cuts" and ignore_ends_len == 15 and depth == 2 ** 32:
        assert one_way == 3 and list(symmetric["whole"])[-2:] == ["a", "b"]


# ---- medium set against the pair-list route ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium():
    """The set, its window pairs and the rows isocon_hw_pairs returns for them (ignore_ends_len 15, every neighbour)."""
    from isocon_amd import end_invariant_functions as END
    from isocon_amd.store import SeqStore
    lst = HC.sorted_list(HC.medium())
    C = {acc: seq for seq, acc in lst}          # (a few of the 600 coincide: the reference asserts one row per candidate)
    seqs = [s for s, _ in lst]
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    q, t = END._window_pairs(lens, 0, len(seqs), 40, 2 ** 32)
    st = SeqStore(seqs)
    try:
        rows = st.hw_pairs(q, t, np.full(len(q), 25, dtype=np.int32))
    finally:
        st.close()
    return {"C": C, "lst": lst, "seqs": seqs, "lens": lens, "q": q, "t": t, "rows": rows}


def test_medium_set_equals_pair_list_route(medium, monkeypatch):
    from isocon_amd import end_invariant_functions as END
    assert len(medium["q"]) > 2048
    new = END.get_NN_graph_ignored_ends_edlib(medium["C"], params_of(15, 2 ** 32))
    new_directed = END.get_all_NN_under_ignored_edge_ends(medium["lst"], params_of(15, 2 ** 32))
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "hw_host_graph")
    old = END.get_NN_graph_ignored_ends_edlib(medium["C"], params_of(15, 2 ** 32))
    old_directed = END.get_all_NN_under_ignored_edge_ends(medium["lst"], params_of(15, 2 ** 32))
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
    assert new == old and rows_of(new) == rows_of(old)
    assert new_directed == old_directed and rows_of(new_directed) == rows_of(old_directed)
    assert sum(len(r) for r in new.values()) > sum(len(r) for r in new_directed.values()) > 1000
    ctr = counters_of(medium["lst"], 15, 2 ** 32, True)
    ed = END._ends_adjusted(medium["rows"], medium["lens"][medium["t"]], 15)
    assert ctr["pairs"] == len(medium["q"])
    assert ctr["hits"] == int((medium["rows"][:, 0] >= 0).sum())
    assert ctr["directed"] == int(((ed >= 0) & (ed <= 10)).sum())
    assert ctr["need_kernel"] == int((medium["lens"][medium["t"]] - medium["lens"][medium["q"]] >= -25).sum())
    assert ctr["kernel_ms"] > 0


def test_hw_pairs_rows_unchanged_by_the_split(medium):
    """isocon_hw_pairs on the explicit pair list (device-built tiles: more than 2 048 pairs) against the oracle on a sample"""
    from oracle import oracle as O
    rng = random.Random(9)
    hits = 0
    for p in rng.sample(range(len(medium["q"])), 200):
        x, y = medium["seqs"][medium["q"][p]], medium["seqs"][medium["t"][p]]
        ed, start, end = O.hw_locate(x, y, 25)
        assert list(medium["rows"][p][:3]) == ([ed, start, end] if ed >= 0 else [-1, -1, -1]), p
        hits += ed >= 0
    assert 10 < hits < 190


# ---- tiny lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [False, True])
def test_tiny_lists(symmetric):
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    rng = random.Random(21)
    s = HC.rnd(rng, 120)
    for seqs in ([], [s], [s[:100], s], [s[:60], s], [s[:50], s[:80], s], [s[:100], s[3:103], s[5:105], s[2:101] + "A"]):
        seqs = sorted(seqs, key=len)
        st = SeqStore(seqs)
        try:
            row_ptr, cols, ed, ctr = st.hw_window_graph(40, 25, 2 ** 32, 15, 10, symmetric, return_counters=True)
        finally:
            st.close()
        lst = [(x, "s%d" % i) for i, x in enumerate(seqs)]
        exp = O.get_NN_graph_ignored_ends_edlib({a: x for x, a in lst}, params_of(15, 2 ** 32)) if symmetric else O.get_all_NN(lst, 0, 0, lst, 2 ** 32, 15)
        got = [("s%d" % i, [("s%d" % t, int(d)) for t, d in zip(cols[row_ptr[i]:row_ptr[i + 1]], ed[row_ptr[i]:row_ptr[i + 1]])]) for i in range(len(seqs))]
        assert got == rows_of(exp)
        lens = [len(x) for x in seqs]
        assert ctr["pairs"] == sum(1 for i in range(len(seqs)) for j in range(len(seqs)) if i != j and abs(lens[i] - lens[j]) <= 40)
        assert len(row_ptr) == len(seqs) + 1 and row_ptr[0] == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def raw_call(st, window, k, cap, symmetric=1):
    from isocon_amd import _lib
    row_ptr = np.zeros(st.n + 1, dtype=np.uint64)
    cols = np.zeros(max(cap, 1), dtype=np.uint32)
    ed = np.zeros(max(cap, 1), dtype=np.int32)
    needed = ctypes.c_uint64(0)
    rc = _lib.lib().isocon_hw_window_graph(st.handle, window, k, 2 ** 32, 15, 10, symmetric, row_ptr.ctypes.data_as(_lib.u64p), cols.ctypes.data_as(_lib.u32p),
                                           ed.ctypes.data_as(_lib.i32p), cap, ctypes.byref(needed), None, None)
    return rc, int(needed.value), row_ptr, cols, ed


def test_refusals_leave_the_store_usable():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    C = HC.family(3)
    seqs = [s for s, _ in HC.sorted_list(C)]
    # more than four symbols
    st = SeqStore(seqs[:-1] + [seqs[-1][:50] + "N" + seqs[-1][51:]])
    try:
        with pytest.raises(_lib.IsoconError) as e:
            st.hw_window_graph(40, 25, 2 ** 32, 15, 10, True)
        assert e.value.status == _lib.ISOCON_E_ALPHABET and "more than four distinct symbols" in str(e.value)
    finally:
        st.close()
    # not in length order
    st = SeqStore(seqs[::-1])
    try:
        with pytest.raises(_lib.IsoconError) as e:
            st.hw_window_graph(40, 25, 2 ** 32, 15, 10, True)
        assert e.value.status == _lib.ISOCON_E_ARG
    finally:
        st.close()
    st = SeqStore(seqs)
    try:
        good = st.hw_window_graph(40, 25, 2 ** 32, 15, 10, True)
        n_edges = len(good[1])
        assert n_edges > 100
        # 513 diagonals
        assert raw_call(st, 40, 236, n_edges)[0] == _lib.ISOCON_E_UNSUPPORTED
        with pytest.raises(_lib.IsoconError) as e:
            st.hw_window_graph(40, 236, 2 ** 32, 15, 10, True)
        assert e.value.status == _lib.ISOCON_E_UNSUPPORTED
        again = st.hw_window_graph(40, 25, 2 ** 32, 15, 10, True)
        assert all((a == b).all() for a, b in zip(good, again))
        # 512 diagonals are served
        assert raw_call(st, 41, 235, 40 * 39)[0] == _lib.ISOCON_OK
        # room for one edge too few, then exactly enough
        rc, needed, row_ptr, _, _ = raw_call(st, 40, 25, n_edges - 1)
        assert rc == _lib.ISOCON_E_CAPACITY and needed == n_edges and (row_ptr.astype(np.int64) == good[0]).all()
        rc, needed, row_ptr, cols, ed = raw_call(st, 40, 25, n_edges)
        assert rc == _lib.ISOCON_OK and needed == n_edges and (cols == good[1]).all() and (ed == good[2]).all()
    finally:
        st.close()


# ---- which route the product takes -----------------------------------------------------------------------------------------------
def test_routing(monkeypatch):
    """Counted at the C ABI: the wrappers themselves stay as they are (a store class with a hw_pairs of its own keeps the pair-list route)."""
    from isocon_amd import _lib
    from isocon_amd import end_invariant_functions as END
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    L = _lib.lib()
    calls = []

    def counted(name):
        real = getattr(L, name)

        def call(*a):
            calls.append(name)
            return real(*a)
        monkeypatch.setattr(L, name, call)

    for name in ("isocon_hw_window_graph", "isocon_hw_pairs", "isocon_hw_pairs_wide"):
        counted(name)
    C = HC.family(4)
    expect = rows_of(O.get_NN_graph_ignored_ends_edlib(C, params_of(15, 2 ** 32)))
    assert rows_of(END.get_NN_graph_ignored_ends_edlib(C, params_of(15, 2 ** 32))) == expect and calls == ["isocon_hw_window_graph"]
    del calls[:]
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "hw_host_graph")
    assert rows_of(END.get_NN_graph_ignored_ends_edlib(C, params_of(15, 2 ** 32))) == expect and calls == ["isocon_hw_pairs"]
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
    del calls[:]
    wide = rows_of(END.get_NN_graph_ignored_ends_edlib(C, params_of(121, 2 ** 32)))
    assert calls == ["isocon_hw_pairs_wide"] and wide == rows_of(O.get_NN_graph_ignored_ends_edlib(C, params_of(121, 2 ** 32)))
    del calls[:]
    # a part of the list, and a list that is not sorted: the pair-list route
    lst = HC.sorted_list(C)
    assert END.get_all_NN(lst[3:9], 3, 3, lst, 2, 5) == O.get_all_NN(lst[3:9], 3, 3, lst, 2, 5) and calls == ["isocon_hw_pairs"]
    del calls[:]
    shuffled = lst[::-1]
    assert END.get_all_NN(shuffled, 0, 0, shuffled, 2 ** 32, 15) == O.get_all_NN(shuffled, 0, 0, shuffled, 2 ** 32, 15) and calls == ["isocon_hw_pairs"]
    del calls[:]
    # a store class that brings its own hw_pairs is served through it
    seen = []
    real_pairs = SeqStore.hw_pairs

    def hw_pairs(self, *a, **kw):
        seen.append(len(a[0]))
        return real_pairs(self, *a, **kw)
    monkeypatch.setattr(SeqStore, "hw_pairs", hw_pairs)
    assert rows_of(END.get_NN_graph_ignored_ends_edlib(C, params_of(15, 2 ** 32))) == expect and len(seen) == 1 and calls == ["isocon_hw_pairs"]
