"""Designed inputs for the edge variants of the statistical test (isocon_amd/csrc/edgevar_core.hpp, edgevar.hpp), shared by the CPU
emulator test (tests/test_edgevar_core.py), the test of the cases themselves (tests/test_edgevar_cases.py) and the GPU test
(tests/test_gpu_edge_variants.py).

A case gives t, c and the two gapped alignments as they are written here: `tc` = (aln_t, aln_c) of the (t, c) alignment, `ct` = (aln_c,
aln_t) of the (c, t) alignment -- the tuples hypothesis_test_module._edge_variants takes.  ops_of_rows turns an alignment into run-length
ops (len << 4 | code, the orientation of SW_alignment_module._ops_to_alignment); the expected values come from _edge_variants and
functions.get_variant_coordinates on the strings."""
import json
import os

from isocon_amd import functions
from isocon_amd import hypothesis_test_module as H

HERE = os.path.dirname(os.path.abspath(__file__))


def filler(n, shift=0):
    """n bases without two equal neighbours (no homopolymer but the ones a case writes itself)"""
    return ("ACGT" * (n // 4 + 3))[shift % 4:shift % 4 + n]


def other(ch):
    """a base that differs from ch and from both neighbours of ch in filler()"""
    return "ACGT"[("ACGT".index(ch) + 2) % 4]


def ops_of_rows(query_row, ref_row):
    """run-length ops of an alignment given as its two gapped rows: '=' / 'X' by the bytes, 'I' where the reference's row is a gap, 'D'
    where the query's is"""
    assert len(query_row) == len(ref_row)
    ops = []
    for q, r in zip(query_row, ref_row):
        assert not (q == "-" and r == "-")
        code = 3 if q == "-" else 2 if r == "-" else 0 if q == r else 1
        if ops and ops[-1] & 15 == code:
            ops[-1] += 16
        else:
            ops.append(16 | code)
    return ops


def mirrored(ops):
    """the ops of the same alignment with the two sequences swapped: 'I' <-> 'D'"""
    return [(op & ~15) | {2: 3, 3: 2}.get(op & 15, op & 15) for op in ops]


def case(name, aln_t, aln_c, ct=None):
    """ct: (aln_c, aln_t) of another alignment of the same two sequences; by default the same alignment"""
    ct = ct or (aln_c, aln_t)
    t, c = aln_t.replace("-", ""), aln_c.replace("-", "")
    assert ct[0].replace("-", "") == c and ct[1].replace("-", "") == t, name
    return {"name": name, "t": t, "c": c, "tc": (aln_t, aln_c), "ct": ct}


def substituted(row, at):
    return "".join(other(ch) if k in at else ch for k, ch in enumerate(row))


def designed_cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))  # noqa: E731
    # ---- no variants and end gaps ----
    add("identical", "ACGTACGTAC", "ACGTACGTAC")
    add("end_gaps_t_leads_c_trails", "---ACGTACGT", "GGAACGTAC--")
    add("end_gaps_c_leads_t_trails", "GGAACGTAC--", "---ACGTACGT")
    add("variant_next_to_masked_runs", "--ACGTACGTAC", "GGTCGTACGA--")
    add("deletion_right_after_masked_run", "--ACGTACGTAC", "GG-CGTACGTAC")
    add("insertion_right_before_masked_run", "ACGTACGT-AC", "ACGTACGTG--")
    # ---- column positions ----
    row = filler(130)
    add("s_at_0_63_64_65_last", row, substituted(row, {0, 63, 64, 65, 129}))
    # ---- 'D' in homopolymers of t ----
    for run in (1, 2, 5):
        for pos in sorted({0, run // 2, run - 1}):
            add("d_run%d_base%d" % (run, pos), "GC" + "A" * run + "CGT", "GC" + "A" * pos + "-" + "A" * (run - pos - 1) + "CGT")
    add("d_run_touches_first_base", "AAACGTAC", "A-ACGTAC")
    add("d_run_touches_last_base", "GTACGAAA", "GTACGA-A")
    left, right = filler(62, 1), filler(40, 1)          # (ends on G, starts with C)
    add("d_run_straddles_64", left + "AAAAA" + right, left + "AA-AA" + right)
    # ---- 'I' and its neighbours in t ----
    add("i_equals_left_run", "GCA-GT", "GCAAGT")
    add("i_equals_right_run", "GC-AGT", "GCAAGT")
    add("i_equals_both_runs", "GCAA-AAGT", "GCAAAAAGT")
    add("i_equals_neither", "GCA-GT", "GCATGT")
    # ---- shared keys ----
    add("two_base_insertion", "ACG--TAC", "ACGCATAC")
    add("two_base_deletion_in_run", "CGAAAATC", "CGA--ATC")
    # ---- snippets past the row's end ----
    add("snippet_past_end", "ACGTC-AAAA", "ACGTCAAAAA")
    # ---- row lengths ----
    add("row_1", "A", "C")
    for n in (63, 64, 65, 129):
        row = filler(n, 2)
        add("row_%d" % n, row, substituted(row, {n // 2, n - 1}))
    # ---- many ops ----
    row = filler(70, 3)
    add("ops_70", row, substituted(row, set(range(1, 70, 2))))
    row = filler(140, 1)
    add("ops_140", row, substituted(row, set(range(1, 140, 2))))
    # ---- capacity: an exon ----
    head, exon, tail = filler(30), filler(400, 2), filler(30, 2)          # (... T | G ... C | G ...)
    add("exon_400", head + exon + tail, head + "-" * 400 + tail)
    # ---- orientation ----
    one_a, one_b, three = ("ACGTTACG", "ACGT-ACG"), ("ACGTTACG", "ACG-TACG"), ("ACGTTACG", "ACGTAC-G")
    add("ct_has_fewer", three[0], three[1], ct=(one_a[1], one_a[0]))
    add("ct_has_as_many", one_a[0], one_a[1], ct=(one_b[1], one_b[0]))
    add("ct_has_more", one_a[0], one_a[1], ct=(three[1], three[0]))
    return out


def ops_of_case(cs):
    """(ops of the (t, c) list, ops of the (c, t) list)"""
    return ops_of_rows(*cs["tc"]), ops_of_rows(*cs["ct"])


def capacity(ops_tc, ops_ct):
    return max(sum(op >> 4 for op in ops if op & 15) for ops in (ops_tc, ops_ct))


def expected_tuple(cs):
    return H._edge_variants(cs["t"], cs["c"], cs["tc"], cs["ct"])


def expected_records(cs):
    """(flipped, [(i, t_last, c_last, key on t, key on c, u_v, type, p_t, p_c, snippet of aln_c, snippet of aln_t)]) in column order: every
    variant by itself through functions.get_variant_coordinates (nothing overwritten)"""
    aln_t, aln_c, variants = H._candidate_vs_reference(cs["tc"], cs["ct"])
    rows = []
    for i, p_t, p_c in variants:
        vt, vc, c2t, t2c = functions.get_variant_coordinates(cs["t"], cs["c"], aln_t, aln_c, [(i, p_t, p_c)])
        (key_t, (v_type, _, u_v)), (key_c, _) = next(iter(vt.items())), next(iter(vc.items()))
        rows.append((i, i - aln_t.count("-", 0, i + 1), i - aln_c.count("-", 0, i + 1), key_t, key_c, u_v, v_type, p_t, p_c, c2t[key_t], t2c[key_c]))
    flipped = len(H._variants_of(cs["ct"][1], cs["ct"][0])) < len(H._variants_of(cs["tc"][0], cs["tc"][1]))
    return flipped, rows


# ---- refusals ----
def refused_ops():
    """[(name, t, c, ops of (t, c), ops of (c, t))]: lists the kernel answers with bad = 1 and no record"""
    aln_t, aln_c = "ACGTTACG--TA", "ACG--ACGCATA"          # (one 'I' run that consumes t only, one 'D' run that consumes c only)
    t, c = aln_t.replace("-", ""), aln_c.replace("-", "")
    good = ops_of_rows(aln_t, aln_c)
    assert good == [3 << 4, 2 << 4 | 2, 3 << 4, 2 << 4 | 3, 2 << 4]
    out = []
    for what, k in (("t", 1), ("c", 3)):
        for name, delta in (("long", 16), ("short", -16)):
            ops = list(good)
            ops[k] += delta
            out.append(("one_%s_of_%s" % (name, what), t, c, ops, mirrored(good)))
    bad_code = list(good)
    bad_code[2] = (bad_code[2] & ~15) | 4
    out.append(("code_4", t, c, bad_code, mirrored(good)))
    out.append(("code_4_in_second_list", t, c, good, mirrored(bad_code)))
    out.append(("empty_op", t, c, good[:2] + [0] + good[2:], mirrored(good)))
    out.append(("no_ops", t, c, [], mirrored(good)))
    return out


def g16_cases():
    """the 70 cases of the reference's fixture g16 as edges: its one alignment as the (t, c) list, its mirror as the (c, t) list (equal
    counts keep (t, c)); expected: the fixture's own variants, variant_coords_t / _c, alignment_c_to_t / _t_to_c"""
    with open(os.path.join(HERE, "golden", "g16_stat_helpers.json")) as f:
        data = json.load(f)
    out = []
    for n, g in enumerate(data["cases"]):
        want = ([tuple(v) for v in g["variants"]],) + tuple(_as_dict(g[k]) for k in ("variant_coords_t", "variant_coords_c", "alignment_c_to_t", "alignment_t_to_c"))
        out.append({"name": "g16_%d" % n, "t": g["t"], "c": g["c"], "tc": (g["aln_t"], g["aln_c"]), "ct": (g["aln_c"], g["aln_t"]), "want": want})
    return out


def _as_dict(pairs):
    """a dict the fixture stores as [[key, value], ...] in its own order; list values are tuples in Python"""
    return {k: tuple(v) if isinstance(v, list) else v for k, v in pairs}


def same_tuple(got, want):
    """equal under == and in the dicts' key order"""
    return got == want and all(list(a.items()) == list(b.items()) for a, b in zip(got[1:], want[1:]))
