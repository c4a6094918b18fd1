"""Cases of the probability queries of the device read tables (isocon_readtab_probability), shared by
tests/test_readtab_probability_core.py (CPU emulator of the lane math) and tests/test_gpu_readtab_probability.py (the kernel through the
C ABI and the Python route).  A case is a table set [(ref_len, read_alignments)], queries [(table index, kind, variant_coords,
snippets)] as in tests/readtab_quality_cases.py, a ccs_dict and one ratio triple per query.  What a query must return comes from the
host: hypothesis_test_module._ccs_probabilities_from_codes on the code bytes of the host tables (QC.table_codes), compared as 64-bit
patterns."""
import random

import numpy as np

import readtab_cases as RC
import readtab_quality_cases as QC
from isocon_amd import hypothesis_test_module as H
from isocon_amd.ccs_info import CCS

RAISED_BY = {QC.Q_BOTH: AssertionError, QC.Q_BEYOND: SystemExit, QC.Q_INDEX: IndexError}
TINY = float(np.finfo(np.float64).tiny)          # the smallest normal double


def ratios_of_sums(subs, ins, dele):
    """the (substitution, insertion, deletion) shares of integer error sums, as functions.get_read_ccs_probabilities_c / _t make them"""
    s, i, d = float(max(1.0, subs)), float(max(1.0, ins)), float(max(1.0, dele))
    tot = s + i + d
    return (s / tot, i / tot, d / tot)


RATIO_SUMS = [(1, 1, 1), (1, 1, 999998), (5, 3, 2), (100, 1, 1), (1, 100, 1), (7, 11, 13), (123456, 789, 1011), (0, 0, 0), (3, 0, 1)]


def status_of_codes(codes):
    """the status word of a query from its (variants, reads) code bytes: 0, or (v + 1) << 8 | byte of what the loop of
    _ccs_probabilities_from_codes meets first -- at a variant the assertion on BOTH, then the exit on BEYOND, then the IndexError, each on
    the reads that no earlier variant has dropped"""
    alive = np.ones(codes.shape[1], dtype=bool)
    for v in range(codes.shape[0]):
        for byte in (QC.Q_BOTH, QC.Q_BEYOND, QC.Q_INDEX):
            if (alive & (codes[v] == byte)).any():
                return ((v + 1) << 8) | byte
        alive &= codes[v] != QC.Q_NEITHER
    return 0


def stepwise(codes, coords, ratios, max_phred_q_trusted):
    """(alive, product) of a query without an event, one variant at a time: every factor is what _ccs_probabilities_from_codes returns for
    that variant alone (1.0 * p_error == p_error), multiplied up in variant order with numpy's doubles.  For products the whole function
    refuses (0.0); equal to it wherever it answers (host_answer asserts that)."""
    n = codes.shape[1]
    alive, prob = np.ones(n, dtype=bool), np.ones(n, dtype=np.float64)
    for v, (i, entry) in enumerate(coords.items()):
        safe = np.where(codes[v] <= 93, codes[v], 0).astype(np.uint8)          # (a dropped read's byte is not looked at)
        _, factor = H._ccs_probabilities_from_codes(n, {i: entry}, lambda *_: safe, ratios, max_phred_q_trusted)
        alive &= codes[v] != QC.Q_NEITHER
        prob = np.where(alive, prob * factor, prob)
    return alive, prob


def host_answer(codes, coords, ratios, max_phred_q_trusted):
    """what isocon_readtab_probability must answer for one query, from the host: (float64 per read, -1.0 where the read is not
    informative; status).  With a status other than 0 the probabilities are None -- the host raises, and this checks that it raises what
    the status says."""
    n = codes.shape[1]
    if len(coords) == 0:
        return np.ones(n, dtype=np.float64), 0
    status = status_of_codes(codes)
    code_of = lambda v, *_: codes[v]  # noqa: E731
    if status:
        try:
            H._ccs_probabilities_from_codes(n, coords, code_of, ratios, max_phred_q_trusted)
        except BaseException as err:          # (SystemExit is none of Exception's)
            assert type(err) is RAISED_BY[status & 255], (status, err)
        else:
            assert n == 0, "the host raises nothing"
        return None, status
    alive, prob = stepwise(codes, coords, ratios, max_phred_q_trusted)
    if n == 0 or ((prob[alive] > 0.0) & (prob[alive] < 1.0)).all():
        whole = H._ccs_probabilities_from_codes(n, coords, code_of, ratios, max_phred_q_trusted)
        assert np.array_equal(whole[0], alive) and np.array_equal(whole[1].view(np.uint64), prob.view(np.uint64))
    return np.where(alive, prob, -1.0), 0


def host_answers(items, queries, ccs, ratios, max_phred_q_trusted, codes=None):
    """codes: per query the (variants, reads) code bytes; those of the host tables unless given"""
    codes = QC.table_codes(items, queries, ccs) if codes is None else codes
    return [host_answer(codes[q], queries[q][2], ratios[q], max_phred_q_trusted) for q in range(len(queries))], codes


def check(got, items, queries, ccs, ratios, max_phred_q_trusted, codes=None):
    """got: per query (float64 per row, status), from the emulator or the device.  Returns (queries with a status, probabilities compared,
    reads not informative)."""
    want, _ = host_answers(items, queries, ccs, ratios, max_phred_q_trusted, codes)
    n_status = n_prob = n_dropped = 0
    for q, ((prob, status), (want_prob, want_status)) in enumerate(zip(got, want)):
        assert status == want_status, (q, queries[q], hex(status), hex(want_status))
        assert len(prob) == len(items[queries[q][0]][1])
        if want_status:
            n_status += 1
            continue
        same = prob.view(np.uint64) == want_prob.view(np.uint64)
        assert same.all(), (q, queries[q], [(float(a).hex(), float(b).hex()) for a, b in zip(prob[~same], want_prob[~same])])
        n_prob += int((want_prob >= 0).sum())
        n_dropped += int((want_prob == -1.0).sum())
    return n_status, n_prob, n_dropped


def with_ratios(rng, queries):
    return [ratios_of_sums(*rng.choice(RATIO_SUMS)) for _ in queries]


def sweep_case():
    """One table of 94 reads equal to their candidate that differ only in the quality at the judged base (0 .. 93); every query is one
    variant there that the read shows on its own row (so the answer is p_error itself): types S, I, D at u_v = 1 and at u_v = 2, both kinds,
    every triple of RATIO_SUMS.  (items, queries, ccs, ratios, [(type, u_v, sums)] per query)"""
    c = "GATTCAGCTA"
    ra = {"q%d" % q: (c, c, ()) for q in range(94)}
    ccs = {"q%d" % q: CCS("q%d" % q, c, [50, 50, 50, 50, q, 50, 50, 50, 50, 50], 1) for q in range(94)}
    queries, ratios, what = [], [], []
    for sums in RATIO_SUMS:
        for kind in (0, 1):
            for v_type in "SID":
                for u_v in (1, 2):
                    queries.append((0, kind, {4: (v_type, "A", u_v)}, {4: "-" * (u_v + 2)}))
                    ratios.append(ratios_of_sums(*sums))
                    what.append((v_type, u_v, sums))
    return [(len(c), ra)], queries, ccs, ratios, what


def sweep_expected(what, max_phred_q_trusted):
    """numpy's own p_error of the 94 qualities for every query of sweep_case"""
    p10 = np.asarray([10 ** (-((q - 3) * (max_phred_q_trusted - 3.0) / (90.0) + 3) / 10.0) for q in range(94)], dtype=np.float64)
    out = []
    for v_type, u_v, sums in what:
        subs_ratio, ins_ratio, del_ratio = ratios_of_sums(*sums)
        if u_v > 1:
            out.append(p10)
        elif v_type == "S":
            out.append((p10 * subs_ratio) / 3.0)
        elif v_type == "I":
            out.append((p10 * ins_ratio) / 4.0)
        else:
            out.append(p10 * del_ratio)
    return out


def long_product_case(max_phred_q_trusted):
    """One table whose reads equal their candidate of 120 bases, with queries of k substitutions (u_v = 1) that every read shows on its own
    row: k is found by multiplying the host's own factor up until the product of the read with quality 93 everywhere is subnormal
    (k_sub), and until it is 0.0 (k_zero).  The second read (quality 0) keeps an ordinary product.  (items, queries [k_sub variants,
    k_zero variants], ccs, ratios, (k_sub, k_zero))"""
    rng = random.Random(41)
    c = "".join(rng.choice("ACGT") for _ in range(120))
    ra = {"hi": (c, c, ()), "lo": (c, c, ())}
    ccs = {"hi": CCS("hi", c, [93] * len(c), 1), "lo": CCS("lo", c, [0] * len(c), 1)}
    ratios = ratios_of_sums(1, 1, 1)
    factor = H._ccs_probabilities_from_codes(1, {0: ("S", "A", 1)}, lambda *_: np.asarray([93], dtype=np.uint8), ratios, max_phred_q_trusted)[1][0]
    p, k, k_sub = np.float64(1.0), 0, None
    while p > 0.0:
        p = p * factor
        k += 1
        if k_sub is None and 0.0 < p < TINY:
            k_sub = k
    k_zero = k
    assert k_sub is not None and k_sub < k_zero <= len(c) - 2
    variants = lambda n: {i: ("S", "A", 1) for i in range(1, n + 1)}  # noqa: E731
    snippets = lambda n: {i: "---" for i in range(1, n + 1)}  # noqa: E731
    queries = [(0, kind, variants(n), snippets(n)) for n in (k_sub, k_zero) for kind in (0, 1)]
    return [(len(c), ra)], queries, ccs, [ratios] * len(queries), (k_sub, k_zero)


def dropped_then_error_case():
    """A read dropped at the second of three variants whose third variant would raise (both sequences shown): it answers -1.0 and the
    query's status stays 0.  (items, queries, ccs, ratios, row of that read)"""
    c = "ACGTACGTACGT"
    ra = {"gone": (c, "ACGTAAGCACGT", ()), "stays": (c, c, ()), "late": (c, "ACGTACGTAGGT", ())}
    ccs = {acc: CCS(acc, v[1], [20 + 3 * j for j in range(len(v[1]))], 1) for acc, v in ra.items()}
    # variant at 1: all three show their own row; at 5: "gone" shows neither; at 9, a variant of the shifted type: "gone" would show its own
    # row and, one column to the left, the snippet ("stays" shows its own row only, "late" neither)
    snippets = {1: "TTT", 5: "TTT", 9: "CAC"}
    queries = [(0, kind, {1: ("S", "A", 1), 5: ("S", "A", 1), 9: (QC.SHIFTED[kind], "A", 1)}, snippets) for kind in (0, 1)]
    return [(len(c), ra)], queries, ccs, [ratios_of_sums(5, 3, 2)] * 2, 0


def status_order_case():
    """Two hand-made tables for the order of events.
    Table 0, 71 rows of a candidate of 6 bases: row 70 raises IndexError at the insertion on base 1 (its read is one base behind three gap
    columns, the record one quality long), row 3 equals the candidate and shows both sequences at the substitution on base 3, every other
    row shows neither there.  Queried with the insertion first (variant 0 in row 70, beyond the first 64-row pass, wins over variant 1 in
    row 3) and with the substitution first.
    Table 1, two rows with a gap column of both rows in front (no alignment has one; the rows are bytes to the tables) and an insertion
    with u_v = 0 on base 0: row 0 shows both, row 1 raises IndexError at the SAME variant: both wins.
    (items, queries, ccs, ratios, expected status words)"""
    c = "ACGTAC"
    ra = {"r%d" % j: (c, c if j == 3 else "---T--" if j == 70 else "ACGTCC", ()) for j in range(71)}
    ccs = {acc: CCS(acc, v[1].replace("-", ""), [40] * len(v[1].replace("-", "")), 1) for acc, v in ra.items()}
    ins, sub = (1, ("I", "A", 1), "--"), (3, ("S", "A", 1), "GTA")
    q_of = lambda order: (0, 1, {i: e for i, e, _ in order}, {i: s for i, _, s in order})  # noqa: E731
    rb = {"x": ("-ACG", "-ACG", ()), "y": ("-ACG", "--C-", ())}
    ccs.update({"x": CCS("x", "ACG", [30, 31, 32], 1), "y": CCS("y", "C", [40], 1)})
    queries = [q_of([ins, sub]), q_of([sub, ins]), (1, 1, {0: ("I", "A", 0)}, {0: "-"})]
    want = [(1 << 8) | QC.Q_INDEX, (1 << 8) | QC.Q_BOTH, (1 << 8) | QC.Q_BOTH]
    return [(6, ra), (3, rb)], queries, ccs, [ratios_of_sums(1, 1, 1)] * 3, want


def directed_case(max_phred_q_trusted):
    """One table set with the directed shapes: the set of QC.directed_case (tables of 0, 1, 64, 65 and 130 rows, queries of 0, 1 and 2
    variants, every error code) and a table of 63 rows, then the tables of long_product_case, dropped_then_error_case and
    status_order_case.  (items, queries, ccs, ratios, marks): marks[name] = (first query, first table) of a named part."""
    rng = random.Random(99)
    items, queries, ccs, _ = QC.directed_case()
    items, queries, ccs = list(items), list(queries), dict(ccs)
    item = RC.table(rng, 45, 63, p_sub=0.03)
    item = (item[0], {"k%d_%s" % (len(items), acc): v for acc, v in item[1].items()})
    queries += QC.queries_for(rng, len(items), item, [{}, {5: ("S", "A", 1)}, {20: ("D", "-", 3), 33: ("I", "G", 2)}])
    ccs.update(QC.records_for(rng, [item[1]]))
    items.append(item)
    ratios = with_ratios(rng, queries)
    marks = {}
    for name, part in (("long", long_product_case(max_phred_q_trusted)), ("dropped", dropped_then_error_case()), ("order", status_order_case())):
        p_items, p_queries, p_ccs, p_ratios = part[:4]
        marks[name] = (len(queries), len(items))
        rename = lambda acc: "%s_%s" % (name, acc)  # noqa: E731
        queries += [(k + len(items), kind, coords, snippets) for k, kind, coords, snippets in p_queries]
        items += [(ref_len, {rename(acc): v for acc, v in ra.items()}) for ref_len, ra in p_items]
        ccs.update({rename(acc): r for acc, r in p_ccs.items()})
        ratios += list(p_ratios)
    return items, queries, ccs, ratios, marks


def random_case(seed):
    """QC.random_case with a ratio triple per query"""
    items, queries, ccs = QC.random_case(seed)
    return items, queries, ccs, with_ratios(random.Random(seed), queries)


def g16_case():
    """all 70 cases of fixture g16 in one table set: (items, queries, ccs, [(want_c, want_t)] per case); the ratios come from the tables"""
    items, queries, ccs, want = [], [], {}, []
    for it, (vt, vc, ac2t, at2c), recs, want_c, want_t in QC.g16_quality_cases():
        queries += [(len(items), 0, vc, at2c), (len(items) + 1, 1, vt, ac2t)]
        items += it
        ccs.update(recs)
        want.append((want_c, want_t))
    return items, queries, ccs, want


def check_g16(got, items, want):
    """the informative reads with repr() of their probabilities and the dropped reads of every case against the reference's own lists"""
    n_prob = n_non = 0
    for n, sides in enumerate(want):
        for side, (want_prob, want_non) in enumerate(sides):
            prob, status = got[2 * n + side]
            accs = list(items[2 * n + side][1])
            assert status == 0 and len(prob) == len(accs)
            assert [[a, repr(float(p))] for a, p in zip(accs, prob) if p >= 0] == want_prob, n
            assert sorted(a for a, p in zip(accs, prob) if p < 0) == sorted(want_non) and all(p == -1.0 for p in prob if p < 0), n
            n_prob += len(want_prob)
            n_non += len(want_non)
    return n_prob, n_non


def trials_case():
    """the 109 trials of RC.stat_trials() as one table set with seeded records (those of tests/test_gpu_readtab_quality.py): (items,
    queries, ccs); the ratios come from the tables"""
    rng = random.Random(7)
    items, queries, ccs = [], [], {}
    for n, (t, c, tc, ct, reads_c, reads_t) in enumerate(RC.stat_trials()):
        rc = {"%d_%s" % (n, a): v for a, v in reads_c.items()}
        rt = {"%d_%s" % (n, a): v for a, v in reads_t.items()}
        for ra in (rc, rt):
            for acc, v in ra.items():
                ccs[acc] = QC.record(rng, acc, v[1].replace("-", ""))
        variants, vt, vc, ac2t, at2c = H._edge_variants(t, c, tc, ct)
        if len(variants) and H._in_range(vc, len(c)) and H._in_range(vt, len(t)):
            queries += [(len(items), 0, vc, at2c), (len(items) + 1, 1, vt, ac2t)]
        items += [(len(c), rc), (len(t), rt)]
    return items, queries, ccs


def table_ratios(tabs, queries):
    """per query the _error_ratios of its edge: the tables of an edge are (2 n, 2 n + 1) in g16_case and trials_case"""
    return [H._error_ratios(tabs[k - k % 2], tabs[k - k % 2 + 1]) for k, _, _, _ in queries]
