"""The designed inputs of tests/msa_cases.py have the properties they were built for (CPU only: the numpy checker of oracle/correction.py
and functions.msa_matrix).  tests/test_gpu_msa_kernels.py runs the same inputs through the HIP kernels; a later edit of a generator that
turns a boundary case into an ordinary one fails here."""
import numpy as np
import pytest

import msa_cases as MC
from oracle import correction as OC

GAP = 45


def _rows(packed, off):
    return [packed[off[r]:off[r + 1]].tobytes() for r in range(len(off) - 1)]


def test_shapes_cover_every_tail():
    cases = MC.correct_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {1, 63, 64, 65, 255, 256, 257, 1000} <= {c[1].shape[1] for c in cases}
    assert {1, 2, 3, 4, 5, 9, 300} <= {c[1].shape[0] for c in cases}
    # each tail together with candidates in its last strip / last workgroup of rows
    for tail_cols in (63, 65, 255, 257, 1000):
        assert any(M.shape[1] == tail_cols and OC.correct_rows(M, deg)[2].sum() > 0 for _, M, deg in cases), tail_cols
    for tail_rows in (2, 3, 5, 9):
        assert any(M.shape[0] == tail_rows and OC.correct_rows(M, deg)[2][-1] > 0 for _, M, deg in cases), tail_rows
    for _, M, deg in cases:
        assert M.dtype == np.uint8 and np.isin(M, MC.SYMS).all() and len(deg) == M.shape[0]


def test_class_totals_helper_is_what_correct_rows_divides_by():
    M = np.frombuffer(b"AC-A" b"AC-A" b"AG-A" b"A-TA" b"ACT-", dtype=np.uint8).reshape(5, 4)
    # column 1: C majority, one substitution, one deletion; column 2: '-' majority, two inserted bases; column 3: one deletion
    assert OC.class_totals(M, np.ones(5)) == (2, 2, 1)
    assert OC.class_totals(M, [3, 1, 1, 1, 1]) == (2, 2, 1)          # (the heavy row agrees with every majority)
    assert OC.class_totals(M, [1, 1, 4, 1, 1]) == (2, 2, 3)          # column 1 now has the majority G (4 : 3 : 1): the three C are substitutions
    maj, unamb = OC.column_majority(M, np.ones(5))
    assert maj.tobytes() == b"AC-A" and unamb.all()


def test_two_way_ties():
    for ncols, seed in ((1, 21), (65, 22)):
        M, deg = MC.two_way_ties(ncols, seed)
        assert (M[0] != M[1]).all()
        maj, unamb = OC.column_majority(M, deg)
        assert not unamb.any()
        first = np.minimum(np.searchsorted(MC.SYMS[:4], M[0]) + 4 * (M[0] == GAP), np.searchsorted(MC.SYMS[:4], M[1]) + 4 * (M[1] == GAP))
        assert (maj == MC.SYMS[np.minimum(first, 4)]).all()          # first maximum in the order A C G T -
        packed, off, n_cand = OC.correct_rows(M, deg)
        assert (n_cand == 0).all() and OC.class_totals(M, deg) == (0, 0, 0)
        assert _rows(packed, off) == [M[r][M[r] != GAP].tobytes() for r in range(2)]


@pytest.mark.parametrize("nr,ncols,seed,sizes", [(5, 65, 23, {2: 30, 5: 1}), (9, 255, 24, {2: 30, 3: 10, 4: 5})])
def test_subset_ties(nr, ncols, seed, sizes):
    M, deg, ties = MC.subset_ties(nr, ncols, seed)
    maj, unamb = OC.column_majority(M, deg)
    assert {k: sum(len(S) == k for _, S in ties) for k in sizes} == sizes
    assert int((~unamb).sum()) == len(ties)
    with_gap = 0
    for col, S in ties:
        cnt = [int((M[:, col] == s).sum()) for s in MC.SYMS]
        assert not unamb[col] and [i for i in range(5) if cnt[i] == max(cnt)] == S
        assert maj[col] == MC.SYMS[S[0]]
        with_gap += 4 in S
    assert with_gap >= 4
    assert OC.correct_rows(M, deg)[2].sum() > 0          # and unambiguous columns with candidates beside them


def test_gap_majority_and_empty_rows():
    for nr, ncols, seed in ((4, 64, 25), (3, 1, 26)):
        M, deg = MC.all_rows_empty(nr, ncols, seed)
        maj, unamb = OC.column_majority(M, deg)
        assert (maj == GAP).all() and unamb.all()
        packed, off, n_cand = OC.correct_rows(M, deg)
        assert n_cand.sum() > 0 and len(packed) == 0 and (off == 0).all()
        c_ins, c_del, c_subs = OC.class_totals(M, deg)
        assert c_ins == n_cand.sum() and c_del == 0 and c_subs == 0
    M, deg = MC.empty_middle_row(5, 257, 27)
    packed, off, n_cand = OC.correct_rows(M, deg)
    assert n_cand.tolist() == [0, 257, 0, 0, 0]
    assert off[1] == off[2] and off[1] > 0 and off[3] > off[2]          # an empty row between non-empty ones


def test_zero_denominators():
    M, deg = MC.only_substitutions(9, 256, 28)
    c_ins, c_del, c_subs = OC.class_totals(M, deg)
    assert (c_ins, c_del) == (0, 0) and c_subs > 50 and OC.correct_rows(M, deg)[2].min() > 0
    M, deg = MC.only_insertions(4, 63, 29)
    c_ins, c_del, c_subs = OC.class_totals(M, deg)
    assert (c_del, c_subs) == (0, 0) and c_ins > 10 and OC.correct_rows(M, deg)[2].sum() == c_ins


@pytest.mark.parametrize("nr,ncols,seed", [(300, 257, 30), (9, 1000, 31)])
def test_heavy_rows(nr, ncols, seed):
    M, deg, heavy = MC.heavy_rows(nr, ncols, seed)
    assert sorted(heavy.values()) == [2, 3, 50] and all(deg[r] == d for r, d in heavy.items()) and (deg != 1).sum() == 3
    maj, unamb = OC.column_majority(M, deg)
    packed, off, n_cand = OC.correct_rows(M, deg)
    rows = _rows(packed, off)
    for r in heavy:
        assert n_cand[r] == 0 and rows[r] == M[r][M[r] != GAP].tobytes()
    # the degree-2 and degree-3 rows disagree with unambiguous majorities (the degree-50 row too where 297 rows outvote it)
    assert all(((M[r] != maj) & unamb).sum() > 0 for r in list(heavy)[:2])
    if nr == 9:          # and here the three together are the majority against the others
        plain = OC.column_majority(M, np.ones(nr))[0]
        assert (plain != maj).sum() > 5


@pytest.mark.parametrize("name", ["noisy_257x513_heavy_rows", "noisy_513x257_heavy_rows"])
def test_row_chunks_and_column_blocks_together(name):
    """a second 256-row chunk of the column counts and a second 256-column block in one matrix, both with a tail; rows of degree 2, 3 and 50 on
    both sides of the chunk boundary; the last chunk's rows change the class totals, the last block's columns hold candidates"""
    M, deg = {c[0]: c[1:] for c in MC.correct_cases()}[name]
    nr, ncols = M.shape
    assert sorted((nr, ncols)) == [257, 513]
    heavy = np.flatnonzero(deg != 1)
    assert sorted(deg[heavy].tolist()) == [2, 3, 50] and heavy.min() < 256 <= heavy.max() and deg[heavy.max()] == 50
    r_last, c_last = 256 * (nr // 256), 256 * (ncols // 256)
    assert 0 < nr - r_last < 256 and 0 < ncols - c_last < 256
    maj, unamb = OC.column_majority(M, deg)
    packed, off, n_cand = OC.correct_rows(M, deg)
    assert (n_cand[heavy] == 0).all() and (n_cand[deg == 1] > 0).all()
    cand = (M != maj) & unamb
    assert cand[deg == 1][:, c_last:].any() and cand[heavy].any()          # (the heavy rows carry errors that are counted, never corrected)
    assert OC.class_totals(M[:r_last], deg[:r_last]) != OC.class_totals(M, deg)
    assert (M[r_last:] != maj)[:, unamb].any()          # (the last chunk's rows put counts into minority symbols)


@pytest.mark.parametrize("name", sorted(MC.TIE_SPECS))
def test_frequency_ties(name):
    spec = MC.TIE_SPECS[name]
    M, deg, want_row, n_corrected = MC.freq_ties(spec, 300, 256, 50)
    assert OC.class_totals(M, deg) == MC.TIE_TOTALS
    packed, off, n_cand = OC.correct_rows(M, deg)
    T = MC.TIE_ROW
    assert n_cand[T] == len(spec)
    assert _rows(packed, off)[T] == want_row.tobytes()          # the checker agrees with exact rational arithmetic
    expect = {"n1": 1, "n2_tied": 2, "n2_apart": 1, "n7_kth_inside_the_tie": 6, "n8_kth_inside_the_tie": 6, "n4_kth_last_of_the_tie": 2, "n3_kth_first_of_the_tie": 3}
    assert n_corrected == expect[name]


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_list_limit_rows(n):
    M, deg = MC.list_limit(n)
    assert M.shape == (5, 4200)
    packed, off, n_cand = OC.correct_rows(M, deg)
    assert n_cand[4] == n and n_cand[:3].tolist() == [0, 0, 0] and 0 < n_cand[3] < 1024
    assert all(t > 100 for t in OC.class_totals(M, deg))
    changed = off[5] - off[4] - int((M[4] != GAP).sum())          # deletions filled minus insertions removed: some, not all
    assert abs(changed) < n // 2


def test_alignment_partitions():
    P = MC.build_partitions()
    assert sorted(P) == sorted(MC.BATCH_ORDER)
    assert [len(P[k].centre) for k in ("L1", "L63_two_rows", "L64_record_codes", "L65_300_rows", "L1023", "L1024", "L1025", "L2049")] == [1, 63, 64, 65, 1023, 1024, 1025, 2049]
    assert P["L63_two_rows"].n_rows == 2 and P["L65_300_rows"].n_rows == 300
    n_ops = sorted(len(o) for p in P.values() for o in p.ops)
    assert {63, 64, 65, 130} <= set(n_ops) and 1 in n_ops
    for k in ("L1", "L64_record_codes", "L65_300_rows", "L2049"):
        assert any(len(o) == 1 and int(o[0]) & 15 == 0 for o in P[k].ops), k          # a member equal to the centre: one '=' op
    ins_len = {len(s) for p in P.values() for _, _, s in p.insertions()}
    assert {1, 2, 31, 32, 33, 70} <= ins_len
    for p in P.values():
        Lm = len(p.centre)
        slots = {t for _, t, _ in p.insertions()}
        if p.name != "L65_300_rows":
            assert 0 in slots or p.name in ("L1024", "L1025", "L2049")
            assert Lm in slots
        M, longest, col_slot = p.host()
        assert M.shape[0] == p.n_rows
        for r in range(p.n_rows):
            assert M[r][M[r] != GAP].tobytes().decode() == p.seqs[r]
    assert {1023, 1024} <= {t for _, t, _ in P["L1024"].insertions()} and {1023, 1024, 1025} <= {t for _, t, _ in P["L1025"].insertions()}
    assert {1023, 1024, 2048, 2049} <= {t for _, t, _ in P["L2049"].insertions()}
    # wide insertions in front of slot 1024 move every later column
    assert P["L2049"].host()[2][1024] > 2 * 1024 and (P["L2049"].host()[1][:1024] > 1).any()
    # two members with different longest insertions of equal length in one slot
    by_slot = {}
    for _, t, s in P["L64_record_codes"].insertions():
        by_slot.setdefault(t, []).append(s)
    assert sorted(by_slot[10]) == ["AC", "G", "GT"] and len({s for s in by_slot[40] if len(s) == 33}) == 2 and len({s for s in by_slot[0] if len(s) == 31}) == 2
    # a deletion run and an insertion across a 64-base word of the member's planes
    a1, a2 = P["L1023"].pairs[1]
    assert a1[60:68] == "-" * 8 and "-" not in a1[:60]
    a1, a2 = P["L1023"].pairs[2]
    assert a2[58:70] == "-" * 12


def test_concatenation_layout():
    P = MC.build_partitions()
    C = MC.Concatenation([P[k] for k in MC.BATCH_ORDER])
    assert [p.n_rows for p in C.parts][:4] == [5, 300, 6, 2]          # tiny, 300 rows, long centre, tiny
    assert C.n_rows == len(C.seqs) == sum(p.n_rows for p in C.parts)
    for i, p in enumerate(C.parts):
        rows, ops, ptr = C.single(i)
        assert ptr[0] == 0 and ptr[1] == 0 and int(ptr[-1]) == len(ops) == sum(len(o) for o in p.ops)
        assert [C.seqs[r] for r in rows] == p.seqs
        for j, o in enumerate(p.ops):
            assert (ops[int(ptr[j + 1]):int(ptr[j + 2])] == o).all()


def test_batched_limit_partitions():
    parts = MC.limit_partitions()
    assert [p.name for p in parts] == ["ordinary0", "limit1024", "ordinary1", "limit1025", "ordinary2", "ordinary3", "ordinary4"]
    seqs = [s for p in parts for s in p.seqs]
    assert len(set(seqs)) == len(seqs)          # (correct_strings keys its partitions by sequence)
    for p in parts:
        M, _, _ = p.host()
        n_cand = OC.correct_rows(M, p.deg)[2]
        if p.name.startswith("limit"):
            n = int(p.name[5:])
            assert n_cand[1] == n and n_cand[0] == 0 and 0 < n_cand[2] < 100 and (n_cand[3:] == 1).all()
            assert len(set(OC.class_totals(M, p.deg))) == 3 and OC.class_totals(M, p.deg)[1] > 100          # deletions among the substitutions
        else:
            assert n_cand.max() < 64 and n_cand.sum() > 0
