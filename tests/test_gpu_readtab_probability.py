"""GPU: the per-read probabilities of the hypothesis tests with base qualities on the device read tables (isocon_readtab_probability:
csrc/readtab.hpp k_rt_probability) through the C ABI and the Python route -- the reference's own probabilities (fixture g16), both
routes on random trials as 64-bit patterns, the quality sweep against numpy's own p_error, directed shapes, the status word and what it
makes the route raise, refusals, and the switch behind do_statistical_tests_per_edge.  Cases: tests/readtab_probability_cases.py, shared
with the CPU emulator test."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_cases as RC  # noqa: E402
import readtab_probability_cases as PC  # noqa: E402
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


def test_reference_fixture():
    """all 70 cases of g16 in one table set, max_phred_q_trusted = 43: the informative reads with repr() of their probabilities and the
    dropped reads as the reference's get_read_ccs_probabilities_c / _t return them -- 527 probabilities, 33 non-informative reads"""
    items, queries, ccs, want = PC.g16_case()
    assert len(want) == 70
    with device_set(items, ccs) as tabs:
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), PC.table_ratios(tabs, queries), 43)
    assert PC.check_g16(got, items, want) == (527, 33)


@pytest.mark.parametrize("max_phred_q_trusted", [43, 30.5])
def test_both_routes_agree_bitwise(max_phred_q_trusted):
    """the 109 trials of the read-table generator and the random tables of seeds 1 and 2: every double equals what
    _ccs_probabilities_from_codes makes of _device_quality's codes -- -1.0 exactly where the read is not informative, the same 64 bits
    elsewhere -- and the status says what that loop raises"""
    assert len(RC.stat_trials()) == 109
    items, queries, ccs = PC.trials_case()
    compared = dropped = 0
    with device_set(items, ccs) as tabs:
        ratios = PC.table_ratios(tabs, queries)
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, max_phred_q_trusted)
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
    n_status, n_prob, n_dropped = PC.check(got, items, queries, ccs, ratios, max_phred_q_trusted, codes)
    assert len(queries) >= 180 and n_prob > 300 and n_dropped > 30, (len(queries), n_status, n_prob, n_dropped)
    for seed in (1, 2):
        items, queries, ccs, ratios = PC.random_case(seed)
        with device_set(items, ccs) as tabs:
            got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, max_phred_q_trusted)
            codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
        n_status, n_prob, n_dropped = PC.check(got, items, queries, ccs, ratios, max_phred_q_trusted, codes)
        compared += n_prob
        dropped += n_dropped
    assert compared > 100 and dropped > 20, (compared, dropped)


@pytest.mark.parametrize("max_phred_q_trusted", [43, 20])
def test_quality_sweep(max_phred_q_trusted):
    """94 reads that differ only in the quality at the judged base: every p_error of S, I, D at u_v = 1 and of u_v = 2, for both kinds
    and nine ratio triples from integer error sums (equal thirds and (1, 1, 999998) among them), is numpy's bit for bit -- the device's
    division by 3.0 and by 4.0"""
    items, queries, ccs, ratios, what = PC.sweep_case()
    assert len({r for r in ratios}) >= 8 and PC.ratios_of_sums(1, 1, 1) in ratios and PC.ratios_of_sums(1, 1, 999998) in ratios
    assert {(kind, w[0], w[1]) for (_, kind, _, _), w in zip(queries, what)} == {(k, t, u) for k in (0, 1) for t in "SID" for u in (1, 2)}
    with device_set(items, ccs) as tabs:
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, max_phred_q_trusted)
    for (prob, status), want, w in zip(got, PC.sweep_expected(what, max_phred_q_trusted), what):
        assert status == 0 and len(prob) == 94
        assert np.array_equal(prob.view(np.uint64), want.view(np.uint64)), (w, [(q, float(a).hex(), float(b).hex()) for q, (a, b) in enumerate(zip(prob, want)) if a != b][:5])


def test_directed_shapes():
    """tables of 0, 1, 63, 64, 65 and 130 rows, queries of 0, 1, 2 and many variants; a read dropped at the second of three variants
    answers -1.0 whatever the third would say; a product that is subnormal on the host and one that is 0.0 there, the variant counts found
    by multiplying the host's own factor up; the latter makes both routes raise AssertionError from _test_on_supporters"""
    items, queries, ccs, ratios, marks = PC.directed_case(43)
    assert {len(ra) for _, ra in items} >= {0, 1, 63, 64, 65, 130}
    assert {len(coords) for _, _, coords, _ in queries} >= {0, 1, 2, 3} and max(len(coords) for _, _, coords, _ in queries) > 50
    with device_set(items, ccs) as tabs:
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, 43)
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
        n_status, n_prob, n_dropped = PC.check(got, items, queries, ccs, ratios, 43)          # (against the host tables' codes)
        assert n_status >= 8 and n_prob > 500 and n_dropped > 100, (n_status, n_prob, n_dropped)
        # the long products
        q0, k0 = marks["long"]
        want, _ = PC.host_answers(items, queries[q0:q0 + 4], ccs, ratios[q0:q0 + 4], 43, codes[q0:q0 + 4])
        tab = tabs[k0]
        for n in (0, 1):          # kind 0, kind 1
            assert 0.0 < want[n][0][0] < PC.TINY and want[2 + n][0][0] == 0.0          # on the host: subnormal, then 0.0
            assert got[q0 + n][0].view(np.uint64).tolist() == want[n][0].view(np.uint64).tolist()
            assert got[q0 + 2 + n][0].view(np.uint64).tolist() == want[2 + n][0].view(np.uint64).tolist()
        # ... as an edge whose c and t are this table (the kind-0 and the kind-1 query of the same variants), through _test_on_supporters
        for qc, qt, raises in ((q0, q0 + 1, False), (q0 + 2, q0 + 3, True)):
            coords, snippets = queries[qc][2], queries[qc][3]
            sup_c, sup_t = H._device_support(tab.set.handle, [(k0, 0, coords, None, tab.n), (k0, 1, coords, snippets, tab.n)])
            results = []
            for work_c, work_t in ((H._SideWork(tab, sup_c, codes[qc]), H._SideWork(tab, sup_t, codes[qt])), (H._SideWork(tab, sup_c, probs=got[qc][0]), H._SideWork(tab, sup_t, probs=got[qt][0]))):
                args = ("ACGT", H._EdgeVariants([("variant",)], coords, coords, snippets, snippets), work_c, work_t, ccs, 43)
                if raises:
                    with pytest.raises(AssertionError):
                        H._test_on_supporters(*args)
                else:
                    results.append(H._test_on_supporters(*args))
            assert raises or (results[0] == results[1] and results[0][2:] == (2, 4))
    # dropped at the second variant, both sequences shown at the third
    q0, _ = marks["dropped"]
    for q in (q0, q0 + 1):
        assert codes[q][:, 0].tolist()[1:] == [QC.Q_NEITHER, QC.Q_BOTH] and codes[q][0, 0] <= 93
        assert got[q][1] == 0 and got[q][0][0] == -1.0 and got[q][0][1] > 0 and got[q][0][2] == -1.0


def _edge_of_case(case):
    """a hand-made edge of QC.raising_cases() as _tests_on_device takes it"""
    _, rc, rt, vc, at2c, vt, ac2t, ccs, raises = case
    bases = lambda ra: len(next(iter(ra.values()))[0].replace("-", "")) if ra else 4  # noqa: E731
    C = {"c": "A" * bases(rc), "t": "A" * bases(rt)}
    return C, {"c": rc, "t": rt}, {("c", "t"): ([("variant",)], vt, vc, ac2t, at2c)}, ccs, raises


@pytest.mark.parametrize("case", QC.raising_cases(), ids=lambda c: c[0])
def test_status_and_what_the_route_raises(case, monkeypatch):
    """every hand-made edge: the status word of its two queries; through _tests_on_device the probability route raises what the codes
    route raises (it sends such an edge through the codes), and where the error sits on a read that an earlier variant dropped the status
    is 0 and the tuple the host tables'"""
    name, rc, rt, vc, at2c, vt, ac2t, ccs, raises = case
    C, partition, variants_of, _, _ = _edge_of_case(case)
    items = [(len(C["c"]), rc), (len(C["t"]), rt)]
    queries = [(0, 0, vc, at2c), (1, 1, vt, ac2t)]
    ratios = [H._error_ratios(H._ReadTable(*items[0]), H._ReadTable(*items[1]))] * 2
    with device_set(items, ccs) as tabs:
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, 43)
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
    want_status = [PC.status_of_codes(c) for c in codes]
    assert [s for _, s in got] == want_status
    byte = {AssertionError: QC.Q_BOTH, SystemExit: QC.Q_BEYOND, IndexError: QC.Q_INDEX}
    if raises is None:
        assert want_status == [0, 0] and {QC.Q_INDEX, QC.Q_BEYOND, QC.Q_BOTH} & set(np.concatenate([c.ravel() for c in codes]).tolist())
        PC.check(got, items, queries, ccs, ratios, 43, codes)
    else:
        assert sorted(want_status)[0] == 0 and sorted(want_status)[1] & 255 == byte[raises] and sorted(want_status)[1] >> 8 >= 1

    def route(variant):
        if variant:
            monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
        else:
            monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
        H.clear_tables()
        before = H.DEVICE_STATS["probability_calls"]
        try:
            return H._tests_on_device([("c", "t")], None, C, partition, ccs, 43, variants_of), H.DEVICE_STATS["probability_calls"] - before
        finally:
            calls.append(H.DEVICE_STATS["probability_calls"] - before)
            H.clear_tables()

    calls = []
    if raises is None:
        host_c, host_t = H._ReadTable(*items[0]), H._ReadTable(*items[1])
        host = H._test_on_supporters(C["t"], H._EdgeVariants([("variant",)], vt, vc, ac2t, at2c), H._SideWork(host_c, np.flatnonzero(host_c.agree_with_candidate(vc))),
                                     H._SideWork(host_t, np.flatnonzero(host_t.show_snippets(vt, ac2t))), ccs, 43)
        assert route(None)[0][("c", "t")] == host and route("stat_host_prob")[0][("c", "t")] == host
    else:
        for variant in (None, "stat_host_prob"):
            with pytest.raises(raises):
                route(variant)
    assert calls == [1, 0]


def test_status_order():
    """an IndexError in row 70 at variant 0 against both sequences shown in row 3 at variant 1: variant 0 wins, across the 64-row passes;
    the variants the other way round; both and IndexError in different rows at the same variant: both wins"""
    items, queries, ccs, ratios, want = PC.status_order_case()
    with device_set(items, ccs) as tabs:
        got = H._device_probability(tabs[0].set.handle, QC.with_rows(items, queries), ratios, 43)
        codes = H._device_quality(tabs[0].set.handle, QC.with_rows(items, queries))
    assert codes[0][0, 70] == QC.Q_INDEX and codes[0][1, 3] == QC.Q_BOTH and sorted(codes[2][0].tolist()) == [QC.Q_INDEX, QC.Q_BOTH]
    assert [s for _, s in got] == want == [PC.status_of_codes(c) for c in codes]
    assert want == [(1 << 8) | 0xFC, (1 << 8) | 0xFE, (1 << 8) | 0xFE]
    PC.check(got, items, queries, ccs, ratios, 43, codes)          # (the host raises what the status says)


def test_refused_arguments():
    ra = {"r0": ("ACG-T", "ACGAT", ()), "r1": ("ACGT", "AC-T", ())}
    items = [(4, ra)]
    ccs = {"r0": QC.CCS("r0", "ACGAT", [10] * 5, 1), "r1": QC.CCS("r1", "ACTA", [10] * 4, 1)}
    ok = [(0, 0, {0: ("S", "A", 1)}, {0: "TT"}), (0, 1, {-4: ("I", "A", 1)}, {-4: "A"})]
    ratios = [PC.ratios_of_sums(1, 1, 1)] * 2
    L = _lib.lib()
    tabs = H._build_device_tables(items)
    dset = tabs[0].set
    try:
        with pytest.raises(_lib.IsoconError, match="bad argument"):          # no qualities attached
            H._device_probability(dset.handle, QC.with_rows(items, ok), ratios, 43)
        assert dset.attach_qualities(ccs)
        got = H._device_probability(dset.handle, QC.with_rows(items, ok), ratios, 43)
        PC.check(got, items, ok, ccs, ratios, 43)
        for i in (4, 5, -5):          # i = ref_len: the per-read statement raises IndexError
            with pytest.raises(_lib.IsoconError, match="bad argument"):
                H._device_probability(dset.handle, QC.with_rows(items, [(0, 0, {i: ("S", "A", 1)}, {i: "GT"})]), ratios[:1], 43)
        # the raw entry: every pointer that must not be NULL, and an output range one slot short (2 rows need 2 doubles)
        q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, _ = H._pack_queries(QC.with_rows(items, ok[:1]))
        q_ratios = np.asarray(ratios[:1], dtype=np.float64)
        base = H._p_of_quality(43)
        out, status = np.full(4, 7.0), np.zeros(1, dtype=np.uint32)

        def call(n_slots=2, **null):
            p = dict(q_table=H._ptr(q_table, _lib.u32p), q_kind=H._ptr(q_kind, _lib.u8p), var_ptr=H._ptr(var_ptr, _lib.u64p), snip_ptr=H._ptr(snip_ptr, _lib.u64p),
                     q_ratios=H._ptr(q_ratios, _lib.f64p), p_of_quality=H._ptr(base, _lib.f64p), prob_ptr=H._ptr(np.asarray([0, n_slots], dtype=np.uint64), _lib.u64p),
                     out_prob=H._ptr(out, _lib.f64p), out_status=H._ptr(status, _lib.u32p))
            p.update({k: None for k in null})
            return L.isocon_readtab_probability(dset.handle, 1, p["q_table"], p["q_kind"], p["var_ptr"], H._ptr(var_pos, _lib.i32p), H._ptr(var_u, _lib.i32p),
                                                H._ptr(var_type, _lib.u8p), p["snip_ptr"], H._ptr(snip_bytes, _lib.u8p), p["q_ratios"], p["p_of_quality"], p["prob_ptr"],
                                                p["out_prob"], p["out_status"], None)

        for name in ("q_table", "q_kind", "var_ptr", "snip_ptr", "q_ratios", "p_of_quality", "prob_ptr", "out_prob", "out_status"):
            assert call(**{name: True}) == E_ARG, name
        assert call(1) == E_ARG and out.tolist() == [7.0] * 4
        assert call(2) == 0 and out[:2].tolist() == got[0][0].tolist() and out[2:].tolist() == [7.0, 7.0]
        assert call(3) == 0 and out[:2].tolist() == got[0][0].tolist() and out[2] == 0.0 and out[3] == 7.0          # the spare slot comes back 0.0
        assert L.isocon_readtab_probability(None, 0, *([None] * 14)) == E_ARG
    finally:
        dset.free()


def _partition():
    """candidates, their reads (stored alignments), the graph c -> t and the reads' records from the first trials of the generator (as in
    tests/test_gpu_readtab_quality.py)"""
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
    ccs = {acc: QC.record(rng, acc, x, prefix="", suffix="") for acc, x in X.items()}
    return C, partition, graph, X, ccs


class _Params(object):
    max_phred_q_trusted = 43


def test_route(monkeypatch):
    """do_statistical_tests_per_edge on a small partition: the default route, ISOCON_DEBUG_VARIANT=stat_host_prob (the codes route) and
    stat_host_tables give equal dicts; the probability entry is called on the default route only, once per table set and round, and every
    route counts one quality call per set and round"""
    C, partition, graph, X, ccs = _partition()
    out, calls = {}, {}
    for variant in (None, "stat_host_prob", "stat_host_tables"):
        if variant:
            monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
        else:
            monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
        assert H.probabilities_on_device_enabled() == (variant is None)
        H.clear_tables()
        before = dict(H.DEVICE_STATS)
        out[variant] = H.do_statistical_tests_per_edge(graph, C, X, partition, ccs, _Params())
        calls[variant] = tuple(H.DEVICE_STATS[k] - before[k] for k in ("create_calls", "quality_attach_calls", "support_calls", "quality_calls", "probability_calls"))
        H.clear_tables()
    assert out[None] == out["stat_host_prob"] == out["stat_host_tables"]
    assert sum(v[0] not in (0.0, 1.0) for row in out[None].values() for v in row.values()) >= 3
    assert calls == {None: (1, 1, 1, 1, 1), "stat_host_prob": (1, 1, 1, 1, 0), "stat_host_tables": (0, 0, 0, 0, 0)}
