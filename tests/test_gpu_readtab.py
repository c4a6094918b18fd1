"""GPU: the device read tables of the hypothesis test (isocon_readtab_create / _support: csrc/readtab.hpp) through the C ABI --
supporting reads as bit sets and per-read error counts against the reference's own results (fixture g16), the per-read statements of
isocon_amd.functions, and hypothesis_test_module._ReadTable on directed shapes; then the cache of table sets behind
do_statistical_tests_per_edge.  Shapes are shared with the CPU emulator test (tests/readtab_cases.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_cases as RC  # noqa: E402
from isocon_amd import _lib  # noqa: E402
from isocon_amd import functions as F  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

pytestmark = pytest.mark.gpu


def run(items, queries):
    """one isocon_readtab_create and one isocon_readtab_support: (errors (n, 3), supporting row indices per query)"""
    tabs = H._build_device_tables(items)          # (at least one table: a set of its own)
    try:
        errors = np.concatenate([np.stack([t.ins, t.dele, t.sub], axis=1) for t in tabs]) if tabs else np.zeros((0, 3), np.int64)
        sup = H._device_support(tabs[0].set.handle, RC.with_rows(items, queries))
        return errors, [s.tolist() for s in sup], tabs
    finally:
        tabs[0].set.free()


def check_case(items, queries):
    want_errors, want_sup = RC.expected(items, queries)
    errors, sup, _ = run(items, queries)
    assert np.array_equal(errors, want_errors)
    for q in range(len(queries)):
        assert sup[q] == want_sup[q], (q, queries[q], sup[q], want_sup[q])
    return sum(len(s) for s in sup)


def test_reference_fixture():
    """all 70 cases of g16 in one table set: supporters in c-then-t order and per-read errors as the reference returns them"""
    cases = RC.g16_cases()
    assert len(cases) == 70
    items, queries = [], []
    for it, qs, _, _ in cases:
        queries += [(len(items) + k, kind, coords, snippets) for k, kind, coords, snippets in qs]
        items += it
    errors, sup, _ = run(items, queries)
    row = 0
    for n, (it, _, support_accs, want_errors) in enumerate(cases):
        assert support_accs != "IndexError"
        accs_c, accs_t = list(it[0][1]), list(it[1][1])
        assert [accs_c[j] for j in sup[2 * n]] + [accs_t[j] for j in sup[2 * n + 1]] == support_accs, n
        by_acc = dict(zip(accs_c + accs_t, errors[row:row + len(accs_c) + len(accs_t)].tolist()))
        assert [[a, by_acc[a]] for a, _ in want_errors] == want_errors, n
        row += len(accs_c) + len(accs_t)
    assert row == len(errors)


def test_random_trials_equal_the_per_read_functions():
    """the generator of test_read_tables_equal_the_per_read_functions on the device path: supporters and errors equal
    functions.get_support / get_read_errors, the test's tuple equals the host tables' (the p-value with ==)"""
    trials = RC.stat_trials()
    assert len(trials) == 109
    items, queries, variants = [], [], []
    for t, c, tc, ct, reads_c, reads_t in trials:
        ev = H._edge_variants(t, c, tc, ct)
        assert H._in_range(ev[2], len(c)) and H._in_range(ev[1], len(t)) and all(i >= 0 for i in list(ev[1]) + list(ev[2]))
        queries += [(len(items), 0, ev[2], None), (len(items) + 1, 1, ev[1], ev[3])]
        items += [(len(c), reads_c), (len(t), reads_t)]
        variants.append(ev)
    errors, sup, tabs = run(items, queries)
    tested = 0
    for n, (t, c, tc, ct, reads_c, reads_t) in enumerate(trials):
        ev = variants[n]
        accs_c, accs_t = list(reads_c), list(reads_t)
        assert [accs_c[j] for j in sup[2 * n]] + [accs_t[j] for j in sup[2 * n + 1]] == F.get_support(reads_c, ev[2], reads_t, ev[1], ev[3]), n
        tab_c, tab_t = tabs[2 * n], tabs[2 * n + 1]
        want = F.get_read_errors(reads_c, reads_t)
        got = dict(zip(accs_t + accs_c, np.stack([np.concatenate([tab_t.ins, tab_c.ins]), np.concatenate([tab_t.dele, tab_c.dele]),
                                                  np.concatenate([tab_t.sub, tab_c.sub])], axis=1).tolist()))
        assert {a: list(v) for a, v in want.items()} == got, n
        fast = H._test_on_supporters(t, ev, H._SideWork(tab_c, np.asarray(sup[2 * n], dtype=np.int64)), H._SideWork(tab_t, np.asarray(sup[2 * n + 1], dtype=np.int64)))
        host = H._test_on_tables(t, c, tc, ct, H._ReadTable(len(c), reads_c), H._ReadTable(len(t), reads_t))
        assert list(host[0].items()) == list(fast[0].items()) and host[1:] == fast[1:], (n, host[1:], fast[1:])
        tested += host[1] not in (0.0, 1.0)
    assert tested > 20


def test_directed_shapes():
    """Row lengths 1, 63, 64, 65, 128, 129, 200; variants on the first and last candidate base (windows clipped at 0 and at len);
    windows across a block boundary; u_v = 70; an end gap run of the candidate's row of more than 64 columns; a snippet whose clipped
    window has the wrong length; coordinates -1 and -ref_len; tables of 0, 1, 64, 65 and 130 rows; empty variant lists; tables of
    different ref_len in one set -- against _ReadTable."""
    items, queries = RC.directed_case()
    assert len({ref_len for ref_len, _ in items}) > 10
    assert check_case(items, queries) > 100


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(seed):
    items, queries = RC.random_case(seed)
    assert check_case(items, queries) > 20


def test_refused_arguments():
    ra = {"r0": ("ACG-T", "ACGAT", ()), "r1": ("ACGT", "AC-T", ())}
    ok = [(4, ra)]
    for i in (4, 5, -5):          # i = ref_len: the per-read statement raises IndexError
        with pytest.raises(_lib.IsoconError, match="bad argument"):
            run(ok, [(0, 0, {i: ("S", "A", 1)}, None)])
        with pytest.raises(_lib.IsoconError, match="bad argument"):
            run(ok, [(0, 1, {0: ("S", "A", 1), i: ("S", "A", 1)}, {0: "AC", i: "AC"})])
    check_case(ok, [(0, 0, {3: ("S", "A", 1)}, None), (0, 0, {-4: ("S", "A", 1)}, None), (0, 1, {-1: ("S", "A", 1)}, {-1: "AT"})])
    with pytest.raises(_lib.IsoconError, match="bad argument"):          # a byte outside ACGT-
        H._build_device_tables([(4, {"r0": ("ACGT", "ANGT", ())})])
    with pytest.raises(_lib.IsoconError, match="bad argument"):
        H._build_device_tables([(4, ra), (4, {"r0": ("ACGT" * 20, "ACGT" * 19 + "ACGn", ())})])
    with pytest.raises(_lib.IsoconError, match="bad argument"):          # rows of one table with 4 and 3 candidate bases
        H._build_device_tables([(4, {"r0": ("ACGT", "ACGT", ()), "r1": ("AC-T", "ACGT", ())})])
    with pytest.raises(ValueError):                                      # rows of unequal length never reach the library
        H._build_device_tables([(4, {"r0": ("ACGT", "ACG", ())})])


def _partition():
    """candidates, their reads (stored alignments) and the graph c -> t from the first trials of the generator"""
    C, partition, graph = {}, {}, {}
    for n, (t, c, _, _, reads_c, reads_t) in enumerate(RC.stat_trials()[:8]):
        C["t%d" % n], C["c%d" % n] = t, c
        partition["c%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_c.items()}
        partition["t%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_t.items()}
        graph["c%d" % n] = {"t%d" % n: 1}
    return C, partition, graph


def test_table_sets_are_cached_between_rounds(monkeypatch):
    """two rounds of do_statistical_tests_per_edge with one candidate's reads changed in between: both rounds equal the host-table
    run, only the changed candidate's table is built again, clear_tables() gives the device memory back"""
    C, partition, graph = _partition()

    def both_paths():
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "stat_host_tables")
        assert not H.device_tables_enabled()
        host = H.do_statistical_tests_per_edge(graph, C, {}, partition, None, object())
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
        assert H.device_tables_enabled()
        before = dict(H.DEVICE_STATS)
        dev = H.do_statistical_tests_per_edge(graph, C, {}, partition, None, object())
        assert dev == host
        return dev, {k: H.DEVICE_STATS[k] - before[k] for k in before}

    H.clear_tables()
    first, stats = both_paths()
    live = [acc for acc in partition if len(partition[acc]) + len(partition[("t" if acc[0] == "c" else "c") + acc[1:]]) > 0]
    assert stats["create_calls"] == 1 and stats["rows_uploaded"] == sum(len(partition[acc]) for acc in live) and stats["support_calls"] == 1
    assert stats["queries"] == len(live)
    assert sum(v[0] not in (0.0, 1.0) for row in first.values() for v in row.values()) >= 3
    held = H.device_table_bytes()
    assert held > 0
    changed = max((acc for acc in partition if acc.startswith("t")), key=lambda acc: len(partition[acc]))
    del partition[changed][next(iter(partition[changed]))]          # the same dict with one read less
    second, stats = both_paths()
    assert stats["create_calls"] == 1 and stats["rows_uploaded"] == len(partition[changed]) and stats["support_calls"] == 2
    assert second != first
    again, stats = both_paths()          # nothing changed: nothing is built
    assert again == second and stats["create_calls"] == 0 and stats["rows_uploaded"] == 0
    assert H.device_table_bytes() > held
    H.clear_tables()
    assert H.device_table_bytes() == 0 and not H._DEVICE_TABLES
