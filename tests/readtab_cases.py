"""Cases of the device read tables (isocon_readtab_*), shared by tests/test_readtab_core.py (CPU emulator of the lane math) and
tests/test_gpu_readtab.py (the kernels through the C ABI).  A case is a table set [(ref_len, read_alignments)] with queries
[(table index, kind, variant_coords, snippets)]; what it must return comes from hypothesis_test_module._ReadTable and
functions.read_errors_from_alignment."""
import json
import os
import random

import numpy as np

from isocon_amd import functions as F
from isocon_amd import hypothesis_test_module as H

HERE = os.path.dirname(os.path.abspath(__file__))


def align_row(rng, c, n_ins=0, p_sub=0.05, p_del=0.03, lead=0, trail=0, lead_read_gap=0):
    """A gapped pair (candidate row, read row): every base of c once, n_ins insertion columns at random places, `lead` / `trail`
    insertion columns at the ends (end gap runs of the candidate's row), the first lead_read_gap bases of c deleted (an end gap run of
    the read's row)."""
    ins_at = sorted(rng.randrange(len(c) + 1) for _ in range(n_ins))
    a, b = ["-"] * lead, [rng.choice("ACGT") for _ in range(lead)]
    for i in range(len(c) + 1):
        for _ in range(ins_at.count(i)):
            a.append("-")
            b.append(rng.choice("ACGT"))
        if i == len(c):
            break
        a.append(c[i])
        r = rng.random()
        if i < lead_read_gap or r < p_del:
            b.append("-")
        elif r < p_del + p_sub:
            b.append(rng.choice([x for x in "ACGT" if x != c[i]]))
        else:
            b.append(c[i])
    a += ["-"] * trail
    b += [rng.choice("ACGT") for _ in range(trail)]
    return "".join(a), "".join(b)


def table(rng, ref_len, n_rows, **kw):
    """(ref_len, {acc: (candidate row, read row, ())}) over one random candidate"""
    c = "".join(rng.choice("ACGT") for _ in range(ref_len))
    ra = {}
    for r in range(n_rows):
        opts = dict(kw)
        if "n_ins" not in opts:
            opts["n_ins"] = rng.randint(0, 4)
        ra["r%d" % r] = align_row(rng, c, **opts) + ((),)
    return ref_len, ra


def window_of(row, kind, v_type, pos, u_v):
    """the window a variant looks at in a read row whose candidate base sits in column pos"""
    before, after = (2, u_v) if v_type == "I" else (1, u_v + 1)
    return row[max(0, pos - before): pos + after]


def column_of(a_row, i):
    return [j for j, ch in enumerate(a_row) if ch != "-"][i]


def queries_for(rng, k, item, coords_list):
    """kind-0 and kind-1 queries on table k for every variant dict of coords_list; a kind-1 snippet is what some row of the table
    shows at that variant (so that rows pass), now and then with a changed letter or a missing one"""
    ref_len, ra = item
    rows = list(ra.values())
    out = []
    for coords in coords_list:
        out.append((k, 0, coords, None))
        snippets = {}
        for i, (v_type, _, u_v) in coords.items():
            if rows:
                a, b = rows[rng.randrange(len(rows))][:2]
                text = window_of(b, 1, v_type, column_of(a, i), u_v)
            else:
                text = "ACG"
            r = rng.random()
            if r < 0.15 and text:
                text = text[:-1]
            elif r < 0.3 and text:
                p = rng.randrange(len(text))
                text = text[:p] + rng.choice("ACGT-") + text[p + 1:]
            snippets[i] = text
        out.append((k, 1, coords, snippets))
    return out


def directed_case():
    """One table set with every directed shape (see tests/test_gpu_readtab.py): (items, queries)."""
    rng = random.Random(2024)
    items, queries = [], []

    def add(item, coords_list):
        items.append(item)
        queries.extend(queries_for(rng, len(items) - 1, item, coords_list))

    # row lengths 1, 63, 64, 65, 128, 129, 200 (rows without insertions: column = position), variants on the first and the last base
    # (windows clipped at 0 and at len), negative coordinates -1 and -ref_len
    for n in (1, 63, 64, 65, 128, 129, 200):
        ends = [{0: ("S", "A", 1)}, {n - 1: ("D", "-", 2)}, {0: ("I", "C", 3), n - 1: ("S", "G", 1)}, {-1: ("S", "A", 1)}, {-n: ("I", "A", 2)},
                {n - 1: ("I", "T", 1)}, {0: ("D", "-", 1)}]
        add(table(rng, n, 3, n_ins=0, p_sub=0.02, p_del=0.02), ends)
    # the same lengths reached with insertions (the column of a position differs from row to row)
    for n in (63, 64, 65, 128, 129, 200):
        ref_len = n - 5
        add(table(rng, ref_len, 4, n_ins=5), [{rng.randrange(ref_len): ("S", "A", 1), rng.randrange(ref_len): ("D", "-", 3)} for _ in range(4)] +
            [{0: ("S", "A", 1), ref_len - 1: ("I", "C", 2)}])
    # windows that straddle a block boundary: positions 62 .. 66 of rows of 100 and 140 columns
    add(table(rng, 100, 8, n_ins=0, p_sub=0.08), [{i: (v, "A", u)} for i in (62, 63, 64, 65, 127 - 64) for v, u in (("S", 1), ("I", 3), ("D", 4))])
    add(table(rng, 134, 8, n_ins=6, p_sub=0.08), [{i: (v, "A", u)} for i in (58, 60, 62, 64, 121, 126) for v, u in (("S", 1), ("I", 3), ("D", 4))])
    # u_v = 70: a homopolymer longer than a mask word; the window runs over three blocks or is cut by the row's end
    add(table(rng, 200, 6, n_ins=3, p_sub=0.004, p_del=0.002), [{i: (v, "A", 70)} for i in (0, 30, 63, 100, 128, 150, 199) for v in "SID"])
    # an end gap run of the candidate's row of more than 64 columns (and of the read's row), before and after the bases
    add(table(rng, 90, 5, n_ins=2, lead=70), [{0: ("S", "A", 1)}, {1: ("I", "A", 2)}, {89: ("D", "-", 2)}, {40: ("S", "A", 1)}])
    add(table(rng, 90, 5, n_ins=2, trail=130, lead_read_gap=66), [{0: ("S", "A", 1)}, {89: ("S", "A", 1)}, {89: ("I", "A", 5)}, {70: ("D", "-", 2)}])
    # a kind-1 snippet whose clipped window has the wrong length: the full-length snippet at the first / last base
    item = table(rng, 50, 4, n_ins=0, p_sub=0.0, p_del=0.0)
    items.append(item)
    k = len(items) - 1
    row = list(item[1].values())[0][1]
    queries += [(k, 1, {0: ("S", "A", 1)}, {0: "A" + row[0:2]}), (k, 1, {0: ("S", "A", 1)}, {0: row[0:2]}),
                (k, 1, {49: ("S", "A", 1)}, {49: row[48:50] + "A"}), (k, 1, {49: ("S", "A", 1)}, {49: row[48:50]}),
                (k, 1, {0: ("I", "A", 1)}, {0: row[0:1]}), (k, 1, {0: ("I", "A", 1)}, {0: "AA" + row[0:1]})]
    # tables of 0, 1, 64, 65 and 130 rows; an empty variant list on each
    for n_rows in (0, 1, 64, 65, 130):
        ref_len = 40 + n_rows % 7
        add(table(rng, ref_len, n_rows, p_sub=0.03), [{}, {5: ("S", "A", 1)}, {20: ("D", "-", 3), 33: ("I", "G", 2)}])
    return items, queries


def random_case(seed, n_tables=12):
    rng = random.Random(seed)
    items, queries = [], []
    for k in range(n_tables):
        ref_len = rng.randint(1, 260)
        item = table(rng, ref_len, rng.randint(0, 9), p_sub=rng.choice([0.0, 0.03, 0.1]), p_del=rng.choice([0.0, 0.03]),
                     lead=rng.choice([0, 0, 3, 70]), trail=rng.choice([0, 0, 2, 65]), lead_read_gap=rng.choice([0, 0, 1]))
        items.append(item)
        coords_list = []
        for _ in range(6):
            coords = {}
            for _ in range(rng.randint(0, 3)):
                coords[rng.randrange(-ref_len, ref_len)] = (rng.choice("SID"), "A", rng.choice([1, 1, 2, 3, 6, 70]))
            coords_list.append(coords)
        queries += queries_for(rng, k, item, coords_list)
    return items, queries


def expected(items, queries):
    """(errors per row as an (n, 3) array, [supporting row indices per query]) from the host statements"""
    errors = [F.read_errors_from_alignment(v[0], v[1]) for _, ra in items for v in ra.values()]
    tabs = [H._ReadTable(ref_len, ra) for ref_len, ra in items]
    sup = []
    for k, kind, coords, snippets in queries:
        ok = tabs[k].show_snippets(coords, snippets) if kind else tabs[k].agree_with_candidate(coords)
        sup.append(np.flatnonzero(ok).tolist())
    return np.asarray(errors, dtype=np.int64).reshape(-1, 3), sup


def with_rows(items, queries):
    """the queries as hypothesis_test_module._pack_queries takes them (the table's row count appended)"""
    return [(k, kind, coords, snippets, len(items[k][1])) for k, kind, coords, snippets in queries]


def g16_cases():
    """fixture g16 (the reference's own get_support / get_read_errors): per case (items = [reads of c, reads of t], queries, the
    accessions in c-then-t order, expected supporters, expected errors in the fixture's order)"""
    g = json.load(open(os.path.join(HERE, "golden", "g16_stat_helpers.json")))
    out = []
    for case in g["cases"]:
        rc = {a: (v[0], v[1], tuple(v[2])) for a, v in case["reads_c"].items()}
        rt = {a: (v[0], v[1], tuple(v[2])) for a, v in case["reads_t"].items()}
        vt = {k: tuple(v) for k, v in case["variant_coords_t"]}
        vc = {k: tuple(v) for k, v in case["variant_coords_c"]}
        ac2t = dict((k, v) for k, v in case["alignment_c_to_t"])
        items = [(len(case["c"]), rc), (len(case["t"]), rt)]
        out.append((items, [(0, 0, vc, None), (1, 1, vt, ac2t)], case["support"], case["errors"]))
    return out


_TRIALS = None


def stat_trials():
    """The generator of tests/test_stat_test.py::test_read_tables_equal_the_per_read_functions (seed 11, 120 trials), made once:
    [(t, c, tc, ct, reads_c, reads_t)] for the trials with c != t."""
    global _TRIALS
    if _TRIALS is not None:
        return _TRIALS
    from oracle import oracle as O
    rng = random.Random(11)

    def mut(b, n, homopolymer=0.5):
        v = list(b)
        for _ in range(n):
            p = rng.randrange(len(v))
            r = rng.random()
            if r < 0.4:
                v[p] = rng.choice("ACGT")
            elif r < 0.7:
                del v[p]
            else:
                v.insert(p, v[p] if rng.random() < homopolymer else rng.choice("ACGT"))
        return "".join(v)

    def aln(a, b, **kw):
        return O.parasail_alignment(a, b, 0, 0, **kw)[2]

    trials = []
    for trial in range(120):
        t = "".join(rng.choice("AACGTT") for _ in range(rng.randint(40, 160)))
        c = mut(t, rng.randint(0, 4))
        if rng.random() < 0.3:
            c = c[rng.randint(0, 6):]
        if rng.random() < 0.3:
            c = c + "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 6)))
        if c == t:
            continue
        reads_c = {"c%d" % k: aln(c, mut(c, rng.randint(0, 4))[rng.randint(0, 3):]) for k in range(rng.randint(0, 7))}
        reads_t = {"t%d" % k: aln(t, mut(t if rng.random() < 0.6 else c, rng.randint(0, 4))) for k in range(rng.randint(0, 9))}
        tc = aln(t, c, opening_penalty=3, mismatch_penalty=-3, gap_ext=1)
        ct = aln(c, t, opening_penalty=3, mismatch_penalty=-3, gap_ext=1)
        trials.append((t, c, tc, ct, reads_c, reads_t))
    _TRIALS = trials
    return trials
