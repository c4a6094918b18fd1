"""GPU: the variants of the hypothesis tests' edges from the alignments' ops on the device (isocon_edge_variants: csrc/edgevar.hpp) -- through
the C ABI on the reference's fixture g16 and the designed cases (tests/edgevar_cases.py, shared with the CPU emulator test), refusals
included; random isoform pairs aligned on the device against the string route; and the Python route behind
do_statistical_tests_per_edge on the FASTA and the FASTQ run of fixture g15 against ISOCON_DEBUG_VARIANT=stat_host_variants."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgevar_cases as EC  # noqa: E402
from isocon_amd import _lib  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402
from isocon_amd import SW_alignment_module as SWM  # noqa: E402
from isocon_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG, E_ALPHABET = -1, -2          # include/isocon_hip.h


def arrays_of(edges):
    """edges [(t, c, ops of (t, c), ops of (c, t))] as _edge_variants_call takes them: (seqs, edge_t, edge_c, ops, ops_ptr)"""
    seqs, index, edge_t, edge_c, ops, ops_ptr = [], {}, [], [], [], [0]
    for t, c, ops_tc, ops_ct in edges:
        for x in (t, c):
            if x not in index:
                index[x] = len(seqs)
                seqs.append(x)
        edge_t.append(index[t])
        edge_c.append(index[c])
        for lst in (ops_tc, ops_ct):
            ops += lst
            ops_ptr.append(len(ops))
    return seqs, edge_t, edge_c, np.asarray(ops, dtype=np.uint32), np.asarray(ops_ptr, dtype=np.uint64)


def rows_of(answer):
    """per edge (bad, flipped, [(i, t_last, c_last, key on t, key on c, u_v, type, p_t, p_c, snippet of aln_c, snippet of aln_t)]) of an
    isocon_edge_variants answer; spare slots must have come back 0"""
    flipped, n_var, bad, recs, snip_ptr, snip_c, snip_t, rec_ptr = answer
    out = []
    for e in range(len(n_var)):
        s0, s1 = int(rec_ptr[e] - rec_ptr[0]), int(rec_ptr[e + 1] - rec_ptr[0])
        rows = []
        for s in range(s0, s0 + int(n_var[e])):
            r = recs[s].tolist()
            assert int(snip_ptr[s + 1] - snip_ptr[s]) == r[6]
            rows.append(tuple(r[:6]) + (chr(r[7] & 255), chr(r[7] >> 8 & 255), chr(r[7] >> 16 & 255), snip_c[int(snip_ptr[s]):int(snip_ptr[s + 1])],
                                        snip_t[int(snip_ptr[s]):int(snip_ptr[s + 1])]))
        assert not recs[s0 + int(n_var[e]):s1].any() and int(snip_ptr[s1]) == int(snip_ptr[s0 + int(n_var[e])])
        out.append((int(bad[e]), int(flipped[e]), rows))
    return out


def as_tuple(rows):
    return H._file_variant_records([(r[0], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10]) for r in rows])


def test_abi_on_the_fixture_and_the_designed_cases():
    """g16 (the reference's own values), the designed cases and the refused lists in ONE call, then in calls of one edge each: every
    array equal, refused lists flagged bad without records, capacities exactly met"""
    cases = EC.g16_cases() + EC.designed_cases()
    edges = [(cs["t"], cs["c"]) + EC.ops_of_case(cs) for cs in cases] + [(t, c, ops_tc, ops_ct) for _, t, c, ops_tc, ops_ct in EC.refused_ops()]
    assert max(EC.capacity(e[2], e[3]) for e in edges) == 400
    before = dict(H.EDGE_VARIANT_STATS)
    together = rows_of(H._edge_variants_call(*arrays_of(edges)))
    assert H.EDGE_VARIANT_STATS["calls"] == before["calls"] + 1 and H.EDGE_VARIANT_STATS["edges"] == before["edges"] + len(edges)
    assert H.EDGE_VARIANT_STATS["kernel_ms"] > before["kernel_ms"]
    alone = [rows_of(H._edge_variants_call(*arrays_of([e])))[0] for e in edges]
    assert together == alone
    for cs, (bad, flipped, rows) in zip(cases, together):
        want_flipped, want_rows = EC.expected_records(cs)
        assert (bad, flipped, rows) == (0, int(want_flipped), want_rows), cs["name"]
        assert EC.same_tuple(as_tuple(rows), cs.get("want") or EC.expected_tuple(cs)), cs["name"]
    assert together[len(cases):] == [(1, 0, [])] * len(EC.refused_ops())
    assert sum(flipped for _, flipped, _ in together) == 1 and {r[6] for _, _, rows in together for r in rows} == {"S", "I", "D"}


def test_abi_refusals():
    L = _lib.lib()
    exon = next(cs for cs in EC.designed_cases() if cs["name"] == "exon_400")
    small = next(cs for cs in EC.designed_cases() if cs["name"] == "two_base_insertion")
    edges = [(cs["t"], cs["c"]) + EC.ops_of_case(cs) for cs in (small, exon)]
    seqs, edge_t, edge_c, ops, ops_ptr = arrays_of(edges)
    error = lambda: L.isocon_last_error().decode()  # noqa: E731
    # a capacity one too small in the second edge
    with pytest.raises(_lib.IsoconError, match="bad argument.*edge 1 has 400 variants, its capacity is 399"):
        H._edge_variants_call(seqs, edge_t, edge_c, ops, ops_ptr, rec_ptr=np.asarray([0, 2, 401], dtype=np.uint64))
    assert [len(rows) for _, _, rows in rows_of(H._edge_variants_call(seqs, edge_t, edge_c, ops, ops_ptr, rec_ptr=np.asarray([0, 2, 402], dtype=np.uint64)))] == [2, 400]
    # an id out of range, descending offsets
    with pytest.raises(_lib.IsoconError, match="bad argument.*sequence id out of range in edge 1"):
        H._edge_variants_call(seqs, edge_t, [edge_c[0], len(seqs)], ops, ops_ptr)
    down = ops_ptr.copy()
    down[3] = down[2] - 1
    with pytest.raises(_lib.IsoconError, match="bad argument.*ops_ptr descends in edge 1"):
        H._edge_variants_call(seqs, edge_t, edge_c, ops, down, rec_ptr=np.asarray([0, 2, 402], dtype=np.uint64))
    with pytest.raises(_lib.IsoconError, match="bad argument.*rec_ptr descends in edge 0"):
        H._edge_variants_call(seqs, edge_t, edge_c, ops, ops_ptr, rec_ptr=np.asarray([5, 2, 402], dtype=np.uint64))
    # a byte outside ACGT
    with_n = [seqs[0][:2] + "N" + seqs[0][3:]] + seqs[1:]
    with pytest.raises(_lib.IsoconError) as refused:
        H._edge_variants_call(with_n, edge_t, edge_c, ops, ops_ptr)
    assert "outside ACGT" in str(refused.value)
    seq_ptr = np.asarray(np.cumsum([0] + [len(x) for x in with_n]), dtype=np.uint64)
    raw = np.frombuffer("".join(with_n).encode(), dtype=np.uint8)
    args = lambda n: (H._ptr(raw, _lib.u8p), H._ptr(seq_ptr, _lib.u64p), len(with_n), n, H._ptr(np.asarray(edge_t, dtype=np.uint32), _lib.u32p),  # noqa: E731
                      H._ptr(np.asarray(edge_c, dtype=np.uint32), _lib.u32p), H._ptr(ops, _lib.u32p), H._ptr(ops_ptr, _lib.u64p), H._ptr(np.asarray([0, 2, 402], dtype=np.uint64), _lib.u64p),
                      H._ptr(np.zeros(2, np.uint8), _lib.u8p), H._ptr(np.zeros(2, np.uint32), _lib.u32p), H._ptr(np.zeros(2, np.uint8), _lib.u8p), H._ptr(np.zeros((402, 8), np.int32), _lib.i32p),
                      H._ptr(np.zeros(403, np.uint64), _lib.u64p), None, None, 0, None, None)
    assert L.isocon_edge_variants(*args(2)) == E_ALPHABET and "outside ACGT" in error()
    # no edges: nothing is looked at
    ms = ctypes.c_float(7.0)
    assert L.isocon_edge_variants(None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None, None, 0, None, ctypes.byref(ms)) == 0 and ms.value == 0.0
    assert H._edge_variants_on_device([], {}, np.zeros(0, np.uint32), np.zeros(1, np.int64)) == []
    # snippet buffers that are too small: the size needed comes back, the call repeated with it succeeds (what _edge_variants_call does)
    ok_seq_ptr = np.asarray(np.cumsum([0] + [len(x) for x in seqs]), dtype=np.uint64)
    ok_raw = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    needed = ctypes.c_uint64(0)
    a = list(args(2))
    a[0], a[1], a[17] = H._ptr(ok_raw, _lib.u8p), H._ptr(ok_seq_ptr, _lib.u64p), ctypes.byref(needed)
    assert L.isocon_edge_variants(*a) == _lib.ISOCON_E_CAPACITY and needed.value == 3 * 400 + 3 + 3


def mutated(rng, t):
    """c from t: substitutions, single-base indels inside homopolymers, sometimes a dropped exon"""
    c = list(t)
    for _ in range(rng.randint(0, 4)):
        k = rng.randrange(len(c))
        c[k] = rng.choice([b for b in "ACGT" if b != c[k]])
    for _ in range(rng.randint(0, 4)):
        runs = [k for k in range(1, len(c)) if c[k] == c[k - 1]]
        k = rng.choice(runs)
        if rng.random() < 0.5:
            c.insert(k, c[k])
        else:
            del c[k]
    if rng.random() < 0.3:
        k, n = rng.randrange(30, len(c) - 120), rng.randint(25, 80)
        del c[k:k + n]
    return "".join(c)


def test_random_edges_equal_the_string_route():
    """200 seeded isoform pairs of 300 - 700 bases (c = t with substitutions, homopolymer indels and, for a third, a dropped exon; every
    fourth pair also loses a few bases at an end), aligned both ways on the device: the ops expand to the strings of the string route
    (the guard of the ops-only alignments), and _edge_variants_on_device equals _edge_variants on those strings, dict order included"""
    rng = random.Random(11)
    gen = np.random.Generator(np.random.PCG64(11))
    C, live, pairs = {}, [], []
    for n in range(200):
        t = synth.make_isoforms(gen, rng.randint(300, 700), 1)[0].tobytes().decode("ascii")
        c = mutated(rng, t)
        if n % 4 == 0:
            c = c[rng.randint(0, 6):len(c) - rng.randint(0, 6)]
        if n % 8 == 1:
            t = t[rng.randint(1, 6):]
        C["t%d" % n], C["c%d" % n] = t, c
        live.append(("c%d" % n, "t%d" % n))
        pairs += [(t, c), (c, t)]
    assert all(300 - 130 <= len(x) <= 1100 for x in C.values())
    alignments = SWM._align_pairs(pairs, [-3] * len(pairs), 2, 3, 1)
    ops, ops_ptr = SWM._align_pairs(pairs, [-3] * len(pairs), 2, 3, 1, want_ops=True)
    for p, (x, y) in enumerate(pairs):
        assert SWM._ops_to_alignment(ops[ops_ptr[p]:ops_ptr[p + 1]].tolist(), x, y) == alignments[p][:2], p
    before = dict(H.EDGE_VARIANT_STATS)
    got = H._edge_variants_on_device(live, C, ops, ops_ptr)
    assert H.EDGE_VARIANT_STATS["calls"] == before["calls"] + 1 and H.EDGE_VARIANT_STATS["lazy_expansions"] == before["lazy_expansions"]
    n_var, types, exons, flipped = 0, set(), 0, 0
    for n, e in enumerate(live):
        want = H._edge_variants(C[e[1]], C[e[0]], alignments[2 * n], alignments[2 * n + 1])
        assert EC.same_tuple(got[n], want), (n, got[n], want)
        n_var += len(want[0])
        types |= {v[0] for v in want[1].values()}
        exons += len(want[0]) >= 25
        flipped += len(H._variants_of(alignments[2 * n + 1][1], alignments[2 * n + 1][0])) < len(H._variants_of(*alignments[2 * n][:2]))
    assert n_var > 2000 and types == {"S", "I", "D"} and exons >= 30, (n_var, types, exons, flipped)
    # the same edges in batches of 64: one call per batch
    H.EDGE_VARIANT_BATCH, saved = 64, H.EDGE_VARIANT_BATCH
    try:
        calls = H.EDGE_VARIANT_STATS["calls"]
        assert H._edge_variants_on_device(live, C, ops, ops_ptr) == got and H.EDGE_VARIANT_STATS["calls"] == calls + 4
    finally:
        H.EDGE_VARIANT_BATCH = saved


@pytest.mark.parametrize("name", ["synth_260x700_4iso", "synth_180x450_3iso_fastq"])
def test_rounds_of_the_pipeline(name, tmp_path, monkeypatch):
    """every round of do_statistical_tests_per_edge of the FASTA and the FASTQ run of fixture g15: the default route makes one device call
    per round and builds no gapped string of a candidate pair; under stat_host_variants no device call is made; the p_values of the two
    are repr()-equal"""
    import test_stat_test as TS
    case = next(c for c in TS.G15 if c["name"] == name)
    original = H.do_statistical_tests_per_edge
    rounds = []

    def both_routes(graph, C, X, read_partition, ccs_dict, params):
        assert H.edge_variants_on_device_enabled()
        before = dict(H.EDGE_VARIANT_STATS)
        dev = original(graph, C, X, read_partition, ccs_dict, params)
        mid = dict(H.EDGE_VARIANT_STATS)
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "stat_host_variants")
        try:
            assert not H.edge_variants_on_device_enabled() and H.device_tables_enabled()
            host = original(graph, C, X, read_partition, ccs_dict, params)
        finally:
            monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
        assert H.EDGE_VARIANT_STATS == mid          # no device call, no expansion
        assert repr(dev) == repr(host)
        live = sum(len(read_partition[c]) + len(read_partition[t]) > 0 for c in graph for t in graph[c])
        assert mid["calls"] - before["calls"] == (1 if live else 0) and mid["edges"] - before["edges"] == live
        assert mid["lazy_expansions"] == before["lazy_expansions"]
        rounds.append((live, bool(ccs_dict), sum(v[0] not in (0.0, 1.0) for row in dev.values() for v in row.values())))
        return dev

    monkeypatch.setattr(H, "do_statistical_tests_per_edge", both_routes)
    assert TS.same_up_to_float_digits(TS.run(case, tmp_path), case["expect"])
    assert len(rounds) >= 2 and sum(r[0] for r in rounds) >= 3 and sum(r[2] for r in rounds) >= 1, rounds
    assert all(r[1] == name.endswith("_fastq") for r in rounds)


def test_lazy_alignments_expand_on_demand():
    """an edge whose variant coordinate the per-read statement cannot index stays on the host tables: its gapped strings are made from the
    ops then, and only its"""
    t, c = "ACGTACGTTGCA", "ACGTACGATGCA"
    pairs = [(t, c), (c, t)]
    ops, ops_ptr = SWM._align_pairs(pairs, [-3, -3], 2, 3, 1, want_ops=True)
    lazy = H._LazyAlignments([("c", "t")], {"t": t, "c": c}, ops, ops_ptr)
    before = H.EDGE_VARIANT_STATS["lazy_expansions"]
    assert ("c", "t") in lazy and ("t", "c") not in lazy and H.EDGE_VARIANT_STATS["lazy_expansions"] == before
    strings = SWM._align_pairs(pairs, [-3, -3], 2, 3, 1)
    assert lazy[("c", "t")] == (strings[0][:2], strings[1][:2]) and lazy[("c", "t")] is lazy[("c", "t")]
    assert H.EDGE_VARIANT_STATS["lazy_expansions"] == before + 1
