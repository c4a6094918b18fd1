"""GPU: the hypothesis tests with base qualities on the device read tables (isocon_readtab_set_qualities / _quality: csrc/readtab.hpp)
through the C ABI and the Python route -- the reference's own probabilities (fixture g16), random trials against both host routes
(the read tables and the per-read functions), directed shapes at the code-byte level, refusals, and the cache of table sets and their
attached qualities behind do_statistical_tests_per_edge.  Shapes are shared with the CPU emulator test (tests/readtab_quality_cases.py)."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_cases as RC  # noqa: E402
import readtab_quality_cases as QC  # noqa: E402
from isocon_amd import _lib  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG = -1          # ISOCON_E_ARG (include/isocon_hip.h)


class device_set(object):
    """one table set with the qualities of ccs attached; freed on exit"""

    def __init__(self, items, ccs):
        self.items, self.ccs = items, ccs

    def __enter__(self):
        self.tabs = H._build_device_tables(self.items)
        assert self.tabs[0].set.attach_qualities(self.ccs)
        return self.tabs

    def __exit__(self, *_):
        self.tabs[0].set.free()


def codes_of(items, queries, ccs):
    with device_set(items, ccs) as tabs:
        return H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))


def check_case(items, queries, ccs):
    got = codes_of(items, queries, ccs)
    want = QC.expected_codes(items, queries, ccs)
    host = QC.table_codes(items, queries, ccs)
    for q in range(len(queries)):
        assert np.array_equal(got[q], want[q]), (q, queries[q], got[q].tolist(), want[q].tolist())
        assert np.array_equal(host[q], want[q]), (q, queries[q])
    return np.concatenate([g.ravel() for g in got]), want


def test_reference_fixture():
    """all 70 cases of g16 in one table set, its `qual` as the records: the informative reads, repr() of their probabilities and the
    dropped reads as the reference's get_read_ccs_probabilities_c / _t return them"""
    cases = QC.g16_quality_cases()
    assert len(cases) == 70
    items, queries, ccs = [], [], {}
    for it, (vt, vc, ac2t, at2c), recs, _, _ in cases:
        queries += [(len(items), 0, vc, at2c), (len(items) + 1, 1, vt, ac2t)]
        items += it
        ccs.update(recs)
    with device_set(items, ccs) as tabs:
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
        n_prob = n_non = 0
        for n, (it, (vt, vc, ac2t, at2c), _, want_c, want_t) in enumerate(cases):
            tab_c, tab_t = tabs[2 * n], tabs[2 * n + 1]
            sums = [float(max(1.0, int(getattr(tab_t, e).sum() + getattr(tab_c, e).sum()))) for e in ("sub", "ins", "dele")]
            ratios = tuple(x / sum(sums) for x in sums)
            ev = H._EdgeVariants([("variant",)], vt, vc, ac2t, at2c)
            for side, tab, code, want in ((H._SIDE_C, tab_c, codes[2 * n], want_c), (H._SIDE_T, tab_t, codes[2 * n + 1], want_t)):
                alive, prob = H._ccs_probabilities_on_table(side, H._SideWork(tab, codes=code), ev, ccs, ratios, 43)
                assert [[a, repr(float(p))] for a, p, ok in zip(tab.accs, prob, alive) if ok] == want[0], n
                assert sorted(a for a, ok in zip(tab.accs, alive) if not ok) == sorted(want[1]), n
                n_prob += len(want[0])
                n_non += len(want[1])
    assert (n_prob, n_non) == (527, 21 + 12)          # the fixture's non-informative reads: 21 of c, 12 of t


def test_random_trials_equal_both_host_routes():
    """the 109 trials of the read-table generator with seeded records (a random prefix of 0, 0, 3 or 7 bases, the read, a suffix of 0, 0
    or 2 bases; qualities uniform over 0 .. 93): the device tuple == the host read tables' == the per-read functions'"""
    trials = RC.stat_trials()
    assert len(trials) == 109
    rng = random.Random(7)
    C, partition, graph, ccs = {}, {}, {}, {}
    for n, (t, c, tc, ct, reads_c, reads_t) in enumerate(trials):
        C["t%d" % n], C["c%d" % n] = t, c
        partition["c%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_c.items()}
        partition["t%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_t.items()}
        for ra in (partition["c%d" % n], partition["t%d" % n]):
            for acc, v in ra.items():
                ccs[acc] = QC.record(rng, acc, v[1].replace("-", ""))
    shifted = sum(r.seq.index(v[1].replace("-", "")) > 0 for ra in partition.values() for acc, v in ra.items() for r in [ccs[acc]])
    live = [("c%d" % n, "t%d" % n) for n in range(len(trials))]
    of_edge = {e: (trials[n][2], trials[n][3]) for n, e in enumerate(live)}
    H.clear_tables()
    before = dict(H.DEVICE_STATS)
    try:
        dev = H._tests_on_device(live, of_edge, C, partition, ccs, 43)
    finally:
        H.clear_tables()
    assert H.DEVICE_STATS["quality_calls"] == before["quality_calls"] + 1 and H.DEVICE_STATS["quality_attach_calls"] == before["quality_attach_calls"] + 1
    tested = dropped = 0
    for n, (t, c, tc, ct, reads_c, reads_t) in enumerate(trials):
        rc, rt = partition["c%d" % n], partition["t%d" % n]
        host = H._test_on_tables(t, c, tc, ct, H._ReadTable(len(c), rc), H._ReadTable(len(t), rt), ccs, 43)
        slow = H._test_on_alignments(t, c, tc, ct, rc, rt, ccs, 43)
        got = dev[live[n]]
        assert list(got[0].items()) == list(host[0].items()) and got[1:] == host[1:], (n, got[1:], host[1:])
        assert got[0] == slow[0] and (got[1], got[2], got[3]) == (slow[1], len(slow[2]), slow[3]), (n, got[1:], slow[1:])
        tested += got[1] not in (0.0, 1.0)
        dropped += len(got[0]) > 0 and got[3] < len(rc) + len(rt)
    assert tested >= 60 and dropped >= 30 and shifted >= 100, (tested, dropped, shifted)


def test_directed_shapes():
    """Code bytes against the restatement of functions._ccs_probabilities and against _ReadTable: row lengths 1, 63, 64, 65, 128, 129; a
    variant on the first and on the last candidate base; pos in columns 63 and 64; u_v = 70; seen = 0 (the read's row opens with 70 gap
    columns: read_coord = -1 is the record's last quality); coord == rec_len falling back on the last base; a record that is too short
    (0xFD); a coordinate below -rec_len (0xFC); both sequences shown (0xFE); qualities 0 and 93; tables of 0, 1, 64, 65 and 130 rows in
    one set; empty variant lists; kinds 0 and 1 with all three variant types."""
    items, queries, ccs, marks = QC.directed_case()
    assert {len(ra) for _, ra in items} >= {0, 1, 64, 65, 130} and any(len(coords) == 0 for _, _, coords, _ in queries)
    assert {(kind, v[0]) for _, kind, coords, _ in queries for v in coords.values()} == {(k, v) for k in (0, 1) for v in "SID"}
    assert {len(v[0]) for _, ra in items for v in ra.values()} >= {1, 63, 64, 65, 128, 129}
    assert any(v[2] == 70 for _, _, coords, _ in queries for v in coords.values())
    codes, want = check_case(items, queries, ccs)
    at = lambda name: [int(want[q][v, j]) for q, v, j in marks[name]]  # noqa: E731
    assert at("seen_0") == [93, 93] and at("coord_is_rec_len") == [0] and at("beyond") == [QC.Q_BEYOND] and at("index") == [QC.Q_INDEX]
    assert at("both") == [QC.Q_BOTH] * 2 and at("quality_0") == [0] and at("quality_93") == [93]
    counts = {c: int((codes == c).sum()) for c in (QC.Q_INDEX, QC.Q_BEYOND, QC.Q_BOTH, QC.Q_NEITHER)}
    assert all(counts.values()) and int((codes <= 93).sum()) > 500, counts


@pytest.mark.parametrize("seed", [1, 2])
def test_random_tables(seed):
    items, queries, ccs = QC.random_case(seed)
    codes, _ = check_case(items, queries, ccs)
    assert int((codes <= 93).sum()) > 50 and int((codes == QC.Q_NEITHER).sum()) > 10


@pytest.mark.parametrize("case", QC.raising_cases(), ids=lambda c: c[0])
def test_error_codes_raise_only_on_informative_reads(case):
    """0xFD -> SystemExit, 0xFC -> IndexError, 0xFE -> AssertionError when the read is still informative at that variant, as on the host
    tables; on a read that an earlier variant dropped nothing is raised and the tuple equals the host route's"""
    _, rc, rt, vc, at2c, vt, ac2t, ccs, raises = case
    items = [(len(next(iter(rc.values()))[0].replace("-", "")) if rc else 4, rc), (len(next(iter(rt.values()))[0].replace("-", "")) if rt else 4, rt)]
    queries = [(0, 0, vc, at2c), (1, 1, vt, ac2t)]
    host_c, host_t = H._ReadTable(items[0][0], rc), H._ReadTable(items[1][0], rt)
    ev = H._EdgeVariants([("variant",)], vt, vc, ac2t, at2c)
    sup_c, sup_t = np.flatnonzero(host_c.agree_with_candidate(vc)), np.flatnonzero(host_t.show_snippets(vt, ac2t))

    def on_host():
        return H._test_on_supporters("ACGT", ev, H._SideWork(host_c, sup_c), H._SideWork(host_t, sup_t), ccs, 43)

    with device_set(items, ccs) as tabs:
        dsup = H._device_support(tabs[0].set.handle, RC.with_rows(items, [(0, 0, vc, None), (1, 1, vt, ac2t)]))
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))

        def on_device():
            return H._test_on_supporters("ACGT", ev, H._SideWork(tabs[0], dsup[0], codes[0]), H._SideWork(tabs[1], dsup[1], codes[1]), ccs, 43)

        if raises is None:
            assert {QC.Q_INDEX, QC.Q_BEYOND, QC.Q_BOTH} & set(np.concatenate([c.ravel() for c in codes]).tolist())          # (the error code is there)
            assert on_device() == on_host()
        else:
            with pytest.raises(raises):
                on_host()
            with pytest.raises(raises):
                on_device()


def test_refused_arguments():
    ra = {"r0": ("ACG-T", "ACGAT", ()), "r1": ("ACGT", "AC-T", ())}
    items = [(4, ra)]
    ccs = {"r0": QC.CCS("r0", "ACGAT", [10] * 5, 1), "r1": QC.CCS("r1", "ACTA", [10] * 4, 1)}          # (what the hand-made arrays below attach)
    ok = [(0, 0, {0: ("S", "A", 1)}, {0: "TT"}), (0, 1, {-4: ("I", "A", 1)}, {-4: "A"})]
    L = _lib.lib()
    tabs = H._build_device_tables(items)
    dset = tabs[0].set
    try:
        with pytest.raises(_lib.IsoconError, match="bad argument"):          # no qualities attached yet
            H._device_quality(dset.handle, QC.with_rows(items, ok))
        qual = np.asarray([10] * 9, dtype=np.uint8)
        qual_ptr = np.asarray([0, 5, 9], dtype=np.uint64)
        start = np.zeros(2, dtype=np.uint32)
        attach = lambda q, p: L.isocon_readtab_set_qualities(dset.handle, H._ptr(q, _lib.u8p), H._ptr(p, _lib.u64p), H._ptr(start, _lib.u32p), None)  # noqa: E731
        bad = qual.copy()
        bad[7] = 94
        assert attach(bad, qual_ptr) == E_ARG                                       # a quality byte 94
        assert attach(qual, np.asarray([0, 5, 4], dtype=np.uint64)) == E_ARG        # a descending qual_ptr
        with pytest.raises(_lib.IsoconError, match="bad argument"):          # (a refused attachment attaches nothing)
            H._device_quality(dset.handle, QC.with_rows(items, ok))
        held = int(L.isocon_readtab_device_bytes(dset.handle))
        assert attach(qual, qual_ptr) == 0 and int(L.isocon_readtab_device_bytes(dset.handle)) > held
        with_one = int(L.isocon_readtab_device_bytes(dset.handle))
        assert attach(qual, qual_ptr) == 0 and int(L.isocon_readtab_device_bytes(dset.handle)) == with_one          # a second call replaces the first
        got = H._device_quality(dset.handle, QC.with_rows(items, ok))
        assert [c.tolist() for c in got] == [c.tolist() for c in QC.expected_codes(items, ok, ccs)] and got[0].tolist() == [[10, 10]]
        for i in (4, 5, -5):          # i = ref_len: the per-read statement raises IndexError
            with pytest.raises(_lib.IsoconError, match="bad argument"):
                H._device_quality(dset.handle, QC.with_rows(items, [(0, 0, {i: ("S", "A", 1)}, {i: "GT"})]))
        # a code buffer that is too small: 2 variants x 2 rows need 4 bytes
        q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, _ = H._pack_queries(QC.with_rows(items, [(0, 0, {1: ("S", "A", 1), 2: ("S", "A", 1)}, {1: "A", 2: "A"})]))
        out = np.zeros(8, dtype=np.uint8)
        call = lambda n: L.isocon_readtab_quality(dset.handle, 1, H._ptr(q_table, _lib.u32p), H._ptr(q_kind, _lib.u8p), H._ptr(var_ptr, _lib.u64p), H._ptr(var_pos, _lib.i32p),  # noqa: E731
                                                  H._ptr(var_u, _lib.i32p), H._ptr(var_type, _lib.u8p), H._ptr(snip_ptr, _lib.u64p), H._ptr(snip_bytes, _lib.u8p),
                                                  H._ptr(np.asarray([0, n], dtype=np.uint64), _lib.u64p), H._ptr(out, _lib.u8p), None)
        assert call(3) == E_ARG and call(4) == 0 and call(6) == 0
    finally:
        dset.free()


def _partition():
    """candidates, their reads (stored alignments), the graph c -> t and the reads' records from the first trials of the generator"""
    rng = random.Random(3)
    C, partition, graph, X = {}, {}, {}, {}
    for n, (t, c, _, _, reads_c, reads_t) in enumerate(RC.stat_trials()[:8]):
        C["t%d" % n], C["c%d" % n] = t, c
        partition["c%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_c.items()}
        partition["t%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_t.items()}
        graph["c%d" % n] = {"t%d" % n: 1}
    for ra in partition.values():
        for acc, v in ra.items():
            X[acc] = v[1].replace("-", "")
    ccs = {acc: QC.record(rng, acc, x, prefix="", suffix="") for acc, x in X.items()}          # (the pipeline's records are cut to the read)
    return C, partition, graph, X, ccs


class _Params(object):
    max_phred_q_trusted = 43


def test_rounds_with_qualities(monkeypatch):
    """rounds of do_statistical_tests_per_edge with a ccs_dict: every round equals the host-table run; a table set is built and its
    qualities attached once, a changed candidate alone is rebuilt and attached, an unchanged round uploads nothing, another ccs_dict
    re-attaches without a rebuild, clear_tables() gives the device memory back"""
    C, partition, graph, X, ccs = _partition()

    def both_paths(ccs_dict):
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "stat_host_tables")
        assert not H.device_tables_enabled()
        host = H.do_statistical_tests_per_edge(graph, C, X, partition, ccs_dict, _Params())
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
        assert H.device_tables_enabled()
        before = dict(H.DEVICE_STATS)
        dev = H.do_statistical_tests_per_edge(graph, C, X, partition, ccs_dict, _Params())
        assert dev == host
        return dev, {k: H.DEVICE_STATS[k] - before[k] for k in before}

    calls = lambda s: (s["create_calls"], s["quality_attach_calls"], s["support_calls"], s["quality_calls"])  # noqa: E731
    H.clear_tables()
    first, stats = both_paths(ccs)
    assert calls(stats) == (1, 1, 1, 1) and stats["kernel_ms"] > 0
    assert sum(v[0] not in (0.0, 1.0) for row in first.values() for v in row.values()) >= 3
    held = H.device_table_bytes()
    assert held > 0
    changed = max((acc for acc in partition if acc.startswith("t")), key=lambda acc: len(partition[acc]))
    del partition[changed][next(iter(partition[changed]))]          # the same dict with one read less
    second, stats = both_paths(ccs)
    assert calls(stats) == (1, 1, 2, 2) and stats["rows_uploaded"] == len(partition[changed])
    assert second != first
    again, stats = both_paths(ccs)          # nothing changed: nothing is built, nothing attached
    assert again == second and calls(stats) == (0, 0, 2, 2) and stats["rows_uploaded"] == 0
    other = {acc: QC.CCS(acc, r.seq, [max(0, q - 1) for q in r.qual], 1) for acc, r in ccs.items()}
    third, stats = both_paths(other)          # other records: both sets attach again, no table is built
    assert calls(stats) == (0, 2, 2, 2) and third != again
    assert H.device_table_bytes() > held
    H.clear_tables()
    assert H.device_table_bytes() == 0 and not H._DEVICE_TABLES
