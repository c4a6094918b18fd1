"""Designed inputs for the consensus-correction kernels (tests/test_gpu_msa_kernels.py compares the device with the checker on them,
tests/test_msa_cases.py asserts on the CPU that every input still has the property it was built for).  Fixed seeds, numpy only.

Matrices (section "correct"): uint8 [n_rows, n_cols] over A C G T - with a degree per row, for isocon_msa_correct.
Alignments (section "build"): a centre, and members made from it by a scripted list of edits, so the gapped strings are known
without an aligner; `Partition` carries them as the host matrix needs them (gapped strings) and as the device needs them (ops)."""
from fractions import Fraction

import numpy as np

from conftest import ops_of_alignment

SYMS = np.frombuffer(b"ACGT-", dtype=np.uint8)
GAP = 45


def _consensus(rng, ncols):
    return SYMS[rng.integers(0, 4, ncols)]


def _other(sym, step=1):
    """another base than `sym` (uint8 arrays or scalars over ACGT)"""
    idx = np.searchsorted(SYMS[:4], sym) if np.ndim(sym) else int(np.flatnonzero(SYMS[:4] == sym)[0])
    return SYMS[(idx + step) % 4]


# ---- 1. matrices for isocon_msa_correct -------------------------------------------------------------------------------------------

def noisy(nr, ncols, seed, heavy=()):
    """a consensus with substitutions, deletions and gap-majority columns with stray bases in about a tenth of the cells;
    heavy: (row, degree) pairs"""
    rng = np.random.default_rng(seed)
    M = np.tile(_consensus(rng, ncols), (nr, 1))
    M[:, rng.random(ncols) < 0.2] = GAP                              # insertion columns: the majority is '-'
    hit = rng.random((nr, ncols)) < 0.1
    M[hit] = SYMS[rng.integers(0, 5, int(hit.sum()))]
    deg = np.ones(nr, dtype=np.int64)
    for r, d in heavy:
        deg[r] = d
    return M, deg


def two_way_ties(ncols, seed):
    """(a) two rows that differ in every column: every column a 1:1 tie"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 5, ncols)
    b = (a + rng.integers(1, 5, ncols)) % 5
    return SYMS[np.stack([a, b])], np.ones(2, dtype=np.int64)


def subset_ties(nr, ncols, seed):
    """(b) every subset of two or more of the five symbols that nr rows can tie on, one column each (the rows in random order): nr = 5 holds
    the pairs (2 : 2 : 1, every third symbol) and the 5-way tie, nr = 9 the pairs (4 : 4 : 1), triples (3 : 3 : 3) and 4-way ties
    (2 : 2 : 2 : 2 : 1); then unambiguous columns (one or two rows off a majority) up to ncols.
    Returns (M, deg, tie_cols: [(column, sorted symbol indices of the tie)])."""
    from itertools import combinations
    rng = np.random.default_rng(seed)
    share = {5: {2: 2, 5: 1}, 9: {2: 4, 3: 3, 4: 2}}[nr]
    cols, ties = [], []
    for k, q in sorted(share.items()):
        for S in combinations(range(5), k):
            rest = [s for s in range(5) if s not in S]
            n_rest = nr - k * q
            for extra in (rest if n_rest else [None]):              # (n_rest is 0 or 1)
                col = [s for s in S for _ in range(q)] + ([extra] if n_rest else [])
                assert len(col) == nr
                ties.append((len(cols), list(S)))
                cols.append(rng.permutation(col))
    assert len(cols) <= ncols
    while len(cols) < ncols:
        col = np.full(nr, rng.integers(0, 5))
        off = rng.choice(nr, rng.integers(1, 3), replace=False)
        col[off] = (col[off] + rng.integers(1, 5)) % 5                # the rows off the majority agree with each other: 1 or 2 < nr - 2
        cols.append(col)
    order = rng.permutation(ncols)
    M = SYMS[np.stack(cols, axis=1)][:, order]
    pos = np.empty(ncols, dtype=np.int64)
    pos[order] = np.arange(ncols)
    return M, np.ones(nr, dtype=np.int64), [(int(pos[c]), S) for c, S in ties]


def all_rows_empty(nr, ncols, seed):
    """(c) every column's majority is '-' and at most one row has a base there: every candidate of a row has frequency 1 / c_ins, all are
    corrected, every corrected row is empty (needs nr >= 3)"""
    rng = np.random.default_rng(seed)
    M = np.full((nr, ncols), GAP, dtype=np.uint8)
    has = rng.random(ncols) < 0.7
    has[0] = True
    M[rng.integers(0, nr, ncols)[has], np.flatnonzero(has)] = SYMS[rng.integers(0, 4, int(has.sum()))]
    return M, np.ones(nr, dtype=np.int64)


def empty_middle_row(nr, ncols, seed):
    """(c) row 1 has bases only where everybody else has '-' (more than half of the columns) and '-' where everybody else has a base:
    its insertions are rarer (1 / c_ins < 1 / c_del) and at least ceil(n / 2) of its candidates, so exactly they are corrected and the row
    becomes empty between non-empty rows (needs nr >= 4)"""
    rng = np.random.default_rng(seed)
    ins = np.zeros(ncols, dtype=bool)
    ins[rng.choice(ncols, ncols // 2 + 8, replace=False)] = True
    M = np.tile(_consensus(rng, ncols), (nr, 1))
    M[:, ins] = GAP
    M[1, ins] = SYMS[rng.integers(0, 4, int(ins.sum()))]
    M[1, ~ins] = GAP
    return M, np.ones(nr, dtype=np.int64)


def only_substitutions(nr, ncols, seed):
    """(d) no '-' anywhere: c_ins = c_del = 0"""
    rng = np.random.default_rng(seed)
    M = np.tile(_consensus(rng, ncols), (nr, 1))
    hit = rng.random((nr, ncols)) < 0.08
    hit[:, 0] = False
    hit[nr - 1, 0] = nr >= 3                                          # (at least one substitution where a majority exists)
    M[hit] = _other(M[hit], rng.integers(1, 4, int(hit.sum())))
    return M, np.ones(nr, dtype=np.int64)


def only_insertions(nr, ncols, seed):
    """(d) columns are unanimous or have a '-' majority with stray bases: c_del = c_subs = 0 (needs nr >= 3)"""
    rng = np.random.default_rng(seed)
    M = np.tile(_consensus(rng, ncols), (nr, 1))
    ins = rng.random(ncols) < 0.5
    ins[0] = True
    M[:, ins] = GAP
    n_ins = int(ins.sum())
    M[rng.integers(0, nr, n_ins), np.flatnonzero(ins)] = SYMS[rng.integers(0, 4, n_ins)]
    return M, np.ones(nr, dtype=np.int64)


def heavy_rows(nr, ncols, seed):
    """(e) rows of degree 2, 3 and 50; the degree-3 row and the degree-2 row carry errors of their own (not candidates, never corrected,
    but counted three and two times), and the three of them together outvote the other rows in some columns"""
    rng = np.random.default_rng(seed)
    M, deg = noisy(nr, ncols, seed)
    heavy = {1: 2, nr // 2: 3, nr - 2: 50}
    for r, d in heavy.items():
        deg[r] = d
    joint = rng.choice(ncols, max(ncols // 20, 1), replace=False)    # 55 of nr + 52 votes: the majority of these columns wherever nr < 58
    sym = SYMS[rng.integers(0, 5, len(joint))]
    for r in heavy:
        M[r, joint] = sym
    return M, deg, heavy


TIE_TOTALS = (21, 18, 12)          # c_ins, c_del, c_subs of freq_ties: 7/21 = 6/18 = 4/12 = 1/3, 14/21 = 2/3, 2/18 = 1/9, 9/18 = 1/2
TIE_SPECS = {                      # candidates (class, own count) of the target row
    "n1": [("S", 1)],
    "n2_tied": [("S", 4), ("D", 6)],
    "n2_apart": [("S", 1), ("D", 6)],
    "n7_kth_inside_the_tie": [("S", 1), ("D", 2), ("S", 4), ("D", 6), ("I", 7), ("S", 4), ("I", 14)],
    "n8_kth_inside_the_tie": [("S", 1), ("D", 2), ("S", 4), ("D", 6), ("I", 7), ("S", 4), ("I", 14), ("D", 9)],
    "n4_kth_last_of_the_tie": [("S", 4), ("D", 6), ("D", 9), ("I", 14)],
    "n3_kth_first_of_the_tie": [("S", 1), ("I", 7), ("D", 6)],
}
TIE_ROW = 5


def freq_ties(spec, nr, ncols, seed):
    """(f) row TIE_ROW gets one candidate per (class, own) of spec: own rows (the target and own - 1 helpers) carry the same minority symbol
    in that column; filler columns, with a single stray symbol in rows away from the target, bring the class totals to TIE_TOTALS exactly;
    unanimous columns fill up to ncols; the columns are shuffled.  Returns (M, deg, the target's corrected row without gaps, how many of its
    candidates are corrected), the last two by exact rational arithmetic."""
    rng = np.random.default_rng(seed)
    T = TIE_ROW
    assert nr >= 2 * 14 + 2 and nr > T + 20
    cols, used = [], {"I": 0, "D": 0, "S": 0}
    for cls, own in spec:
        base = int(rng.integers(0, 4))
        col = np.full(nr, 4 if cls == "I" else base)
        rows = [T] + list(range(T + 1, T + own))
        col[rows] = {"I": base, "D": 4, "S": (base + 1) % 4}[cls]
        cols.append(col)
        used[cls] += own
    for cls, total in zip("IDS", TIE_TOTALS):
        assert used[cls] <= total
        for i in range(total - used[cls]):
            base = int(rng.integers(0, 4))
            col = np.full(nr, 4 if cls == "I" else base)
            col[T + 15 + (i % 5)] = {"I": base, "D": 4, "S": (base + 2) % 4}[cls]
            cols.append(col)
    assert len(cols) <= ncols
    while len(cols) < ncols:
        cols.append(np.full(nr, rng.integers(0, 4)))
    M = SYMS[np.stack(cols, axis=1)]
    # the target row as the rule leaves it, by exact rational arithmetic: the ceil(n / 2)-th smallest frequency and everything tied with it
    tot = dict(zip("IDS", TIE_TOTALS))
    f = [Fraction(own, tot[cls]) for cls, own in spec]
    thr = sorted(f)[(len(f) + 1) // 2 - 1]
    row = M[T].copy()
    for i, (cls, own) in enumerate(spec):
        if f[i] <= thr:
            row[i] = GAP if cls == "I" else M[0, i]          # (row 0 holds the majority of every column)
    order = rng.permutation(ncols)
    row = row[order]
    return M[:, order], np.ones(nr, dtype=np.int64), row[row != GAP], sum(x <= thr for x in f)


def list_limit(n_cand, ncols=4200, seed=3):
    """(g) five rows; four equal, the fifth differs from them in its first n_cand columns -- by another base, by '-', or by a base where
    the four have '-' -- and in some of them row 3 carries the same symbol as row 4 (own count 2, still 3 : 2), so that row 4's frequencies
    take six values"""
    rng = np.random.default_rng(seed)
    M = np.tile(_consensus(rng, ncols), (5, 1))
    kind = rng.integers(0, 3, n_cand)
    c = np.arange(n_cand)
    M[4, c[kind == 0]] = _other(M[4, c[kind == 0]], rng.integers(1, 4, int((kind == 0).sum())))
    M[4, c[kind == 1]] = GAP
    M[:4, c[kind == 2]] = GAP
    shared = c[rng.random(n_cand) < 0.3]
    M[3, shared] = M[4, shared]
    return M, np.ones(5, dtype=np.int64)


def correct_cases():
    """(name, M, deg) of every matrix of section 1.  n_cols 1, 63, 64, 65, 255, 256, 257, 1000 and n_rows 1, 2, 3, 4, 5, 9, 300 all occur,
    and each tail (256-column workgroup, 64-column strip, 4 rows per workgroup) occurs with candidates in it."""
    out = [
        ("noisy_1x1", *noisy(1, 1, 11)),
        ("noisy_1x1000", *noisy(1, 1000, 12)),
        ("noisy_2x64_heavy_centre", *noisy(2, 64, 13, heavy=[(0, 3)])),          # (two rows of degree 1 only ever tie)
        ("noisy_3x63_heavy_centre", *noisy(3, 63, 14, heavy=[(0, 4)])),
        ("noisy_4x255", *noisy(4, 255, 15)),
        ("noisy_5x256", *noisy(5, 256, 16)),
        ("noisy_9x257", *noisy(9, 257, 17, heavy=[(0, 2)])),
        ("noisy_300x1000", *noisy(300, 1000, 18, heavy=[(0, 7)])),
        # more than one 256-row chunk of the column counts AND more than one 256-column block; rows of degree 2, 3, 50 on both sides of the chunk boundary
        ("noisy_257x513_heavy_rows", *noisy(257, 513, 19, heavy=[(0, 2), (255, 3), (256, 50)])),
        ("noisy_513x257_heavy_rows", *noisy(513, 257, 20, heavy=[(255, 2), (256, 3), (511, 50)])),
        ("a_two_way_ties_2x1", *two_way_ties(1, 21)),
        ("a_two_way_ties_2x65", *two_way_ties(65, 22)),
        ("b_subset_ties_5x65", *subset_ties(5, 65, 23)[:2]),
        ("b_subset_ties_9x255", *subset_ties(9, 255, 24)[:2]),
        ("c_all_rows_empty_4x64", *all_rows_empty(4, 64, 25)),
        ("c_all_rows_empty_3x1", *all_rows_empty(3, 1, 26)),
        ("c_empty_middle_row_5x257", *empty_middle_row(5, 257, 27)),
        ("d_only_substitutions_9x256", *only_substitutions(9, 256, 28)),
        ("d_only_insertions_4x63", *only_insertions(4, 63, 29)),
        ("e_heavy_rows_300x257", *heavy_rows(300, 257, 30)[:2]),
        ("e_heavy_rows_9x1000", *heavy_rows(9, 1000, 31)[:2]),
    ]
    for i, (name, spec) in enumerate(sorted(TIE_SPECS.items())):
        out.append(("f_freq_ties_%s_300x%d" % (name, (64, 256, 65, 63, 255, 257, 1000)[i]), *freq_ties(spec, 300, (64, 256, 65, 63, 255, 257, 1000)[i], 40 + i)[:2]))
    for n in (2047, 2048, 2049):
        out.append(("g_list_limit_%d" % n, *list_limit(n)))
    return out


# ---- 2. designed alignments ---------------------------------------------------------------------------------------------------------

def random_seq(rng, n):
    return SYMS[rng.integers(0, 4, n)].tobytes().decode()


def apply_edits(centre, edits):
    """edits: ("X", t) substitution of centre base t; ("D", t, n) the member lacks centre bases t .. t + n - 1; ("I", t, string) the member
    has `string` in slot t (in front of centre base t; t = len(centre): behind the last).  Positions must not overlap.  Returns the gapped
    strings (centre, member)."""
    ins = {}
    what = {}
    for e in edits:
        if e[0] == "I":
            assert e[1] not in ins and 0 <= e[1] <= len(centre)
            ins[e[1]] = e[2]
        else:
            for t in range(e[1], e[1] + (e[2] if e[0] == "D" else 1)):
                assert t not in what and 0 <= t < len(centre)
                what[t] = e[0]
    a1, a2 = [], []
    for t in range(len(centre) + 1):
        if t in ins:
            a1.append("-" * len(ins[t]))
            a2.append(ins[t])
        if t < len(centre):
            a1.append(centre[t])
            a2.append({"X": "ACGT"[("ACGT".index(centre[t]) + 1) % 4], "D": "-", None: centre[t]}[what.get(t)])
    return "".join(a1), "".join(a2)


def n_ops_member(centre, n):
    """edits whose alignment has exactly n ops: n - 1 runs of one base ('=' alternating with a substitution, a 1-base insertion, a
    1-base deletion in turn) and the rest of the centre as one '=' run"""
    edits, t, turn = [], 0, 0
    for i in range(n - 1):
        if i % 2 == (n - 1) % 2:          # '=' (op n - 2 is never '=': the closing run stays an op of its own)
            t += 1
            continue
        kind = "XID"[turn % 3]
        turn += 1
        if kind == "I":
            edits.append(("I", t, "ACGT"[turn % 4]))
        else:
            edits.append(("X", t) if kind == "X" else ("D", t, 1))
            t += 1
    assert t < len(centre)
    return edits


class Partition(object):
    """centre + members as gapped pairs.  host(): (M of functions.msa_matrix, longest, col_slot as the layout defines them);
    ops: per member the run-length ops; seqs: [centre] + member strings."""

    def __init__(self, name, centre, member_edits, degree=1):
        self.name, self.centre, self.degree = name, centre, degree
        self.pairs = [apply_edits(centre, e) for e in member_edits]
        for a1, a2 in self.pairs:
            assert a1.replace("-", "") == centre and len(a1) == len(a2)
        self.members = [a2.replace("-", "") for _, a2 in self.pairs]
        self.ops = [ops_of_alignment(a1, a2) for a1, a2 in self.pairs]
        self.seqs = [centre] + self.members
        self.n_rows = len(self.seqs)
        self.deg = np.ones(self.n_rows, dtype=np.int32)
        self.deg[0] = degree
        self._host = None

    def insertions(self):
        """[(row, slot, string)] read off the gapped strings"""
        out = []
        for r, (a1, a2) in enumerate(self.pairs, 1):
            t = i = 0
            while i < len(a1):
                if a1[i] == "-":
                    j = i
                    while j < len(a1) and a1[j] == "-":
                        j += 1
                    out.append((r, t, a2[i:j]))
                    i = j
                else:
                    t += 1
                    i += 1
        return out

    def host(self):
        if self._host is None:
            from isocon_amd import functions as FUN
            part = {"centre": (0, self.centre, self.centre, self.degree)}
            for i, (a1, a2) in enumerate(self.pairs):
                part["member%d" % i] = (0, a1, a2, 1)
            keys, M = FUN.msa_matrix(self.centre, part)          # (the keys are labels: two rows may spell the same sequence)
            Lm = len(self.centre)
            longest = np.zeros(Lm + 1, dtype=np.int64)
            for _, t, s in self.insertions():
                longest[t] = max(longest[t], len(s))
            width = np.where(longest > 1, longest + 2, 1)
            col_slot = np.zeros(Lm + 1, dtype=np.int64)
            col_slot[1:] = np.cumsum(width[:-1] + 1)
            assert M.shape == (self.n_rows, int(width.sum()) + Lm)
            assert M[0, col_slot[:Lm] + width[:Lm]].tobytes().decode() == self.centre          # the centre's bases sit in the base columns
            self._host = (M, longest, col_slot)
        return self._host


def _light_edits(rng, Lm, wide=True):
    """a few random substitutions, 1-base indels and (wide) 2-3 base insertions at distinct positions"""
    edits = []
    pos = rng.choice(Lm, min(Lm, 8), replace=False).tolist()
    for t in pos[:3]:
        edits.append(("X", t))
    for t in pos[3:5]:
        edits.append(("D", t, 1))
    slots = rng.choice(Lm + 1, 3, replace=False).tolist()
    edits.append(("I", slots[0], random_seq(rng, 1)))
    if wide and rng.random() < 0.5:
        edits.append(("I", slots[1], random_seq(rng, int(rng.integers(2, 4)))))
    return edits


def build_partitions():
    """The partitions of section 2, by name."""
    rng = np.random.default_rng(77)
    P = {}
    c = "G"
    P["L1"] = Partition("L1", c, [[], [("I", 0, "A"), ("I", 1, "CG")], [("X", 0)], [("D", 0, 1), ("I", 1, "T")]], degree=2)
    c = random_seq(rng, 63)          # two rows: insertions in slot 0 and slot Lm, a substitution, a deletion
    P["L63_two_rows"] = Partition("L63_two_rows", c, [[("I", 0, "T"), ("X", 5), ("D", 20, 3), ("I", 63, "GA")]], degree=3)
    c = random_seq(rng, 64)          # lengths 2, 31, 32, 33 around the 32 coded bases; equal longest insertions that differ (slot 10)
    P["L64_record_codes"] = Partition("L64_record_codes", c, [
        [],
        [("I", 0, random_seq(rng, 31)), ("I", 10, "GT"), ("I", 40, random_seq(rng, 33)), ("I", 64, random_seq(rng, 32))],
        [("I", 0, random_seq(rng, 2)), ("I", 10, "AC"), ("I", 40, random_seq(rng, 32)), ("I", 64, random_seq(rng, 33))],
        [("I", 0, random_seq(rng, 31)), ("I", 10, "G"), ("I", 40, random_seq(rng, 33)), ("X", 63)],
        [("I", 30, random_seq(rng, 70)), ("D", 0, 2), ("I", 64, "C")],
    ])
    c = random_seq(rng, 65)          # 300 rows: more than the 256 rows a counting workgroup takes
    P["L65_300_rows"] = Partition("L65_300_rows", c, [[]] + [_light_edits(rng, 65) for _ in range(298)], degree=5)
    c = random_seq(rng, 1023)        # the last slot is the last of the layout scan's first step
    P["L1023"] = Partition("L1023", c, [
        [("I", 0, random_seq(rng, 33)), ("D", 60, 11), ("I", 1023, random_seq(rng, 70))],          # member positions 33 ..: the deletion run sits at a plane word's end
        [("I", 60, random_seq(rng, 8)), ("X", 1022), ("I", 1023, "A")],                            # member positions 60 .. 67 straddle a 64-base word
        [("D", 58, 12), ("I", 1022, "TT")],                                                        # centre bases 58 .. 69 across the word boundary
        n_ops_member(c, 63),
    ])
    c = random_seq(rng, 1024)
    P["L1024"] = Partition("L1024", c, [
        [("I", 1023, "ACG"), ("I", 1024, "T")],
        [("I", 500, random_seq(rng, 5)), ("I", 1023, "A"), ("I", 1024, random_seq(rng, 4)), ("D", 1020, 3)],
        n_ops_member(c, 64),
    ], degree=2)
    c = random_seq(rng, 1025)
    P["L1025"] = Partition("L1025", c, [
        [("I", 100, random_seq(rng, 6)), ("I", 1023, "GG"), ("I", 1024, "C"), ("I", 1025, "TTT")],
        [("I", 1024, random_seq(rng, 31)), ("X", 1024), ("D", 1000, 20)],
        [("I", 1023, "A"), ("I", 1025, "A"), ("X", 0)],
        n_ops_member(c, 65),
    ])
    c = random_seq(rng, 2049)        # three steps of the layout scan, the last with one slot
    P["L2049"] = Partition("L2049", c, [
        [("I", 7, random_seq(rng, 3)), ("I", 1024, "AC"), ("I", 2048, random_seq(rng, 2)), ("I", 2049, random_seq(rng, 33))],
        [("I", 1023, random_seq(rng, 9)), ("D", 1024, 64), ("I", 2047, "G"), ("I", 2049, "T")],
        [("D", 2040, 9)],
        n_ops_member(c, 130),
        [],
    ], degree=4)
    return P


BATCH_ORDER = ["L1", "L65_300_rows", "L2049", "L63_two_rows", "L1024", "L64_record_codes", "L1023", "L1025"]      # tiny, 300 rows, long centre, tiny, ...


class Concatenation(object):
    """partitions laid out for one store and one isocon_msa_build_ops_batch call"""

    def __init__(self, parts):
        self.parts = parts
        self.seqs = [s for p in parts for s in p.seqs]
        self.first_row = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([p.n_rows for p in parts], out=self.first_row[1:])
        self.n_rows = int(self.first_row[-1])
        self.row_ids = np.arange(self.n_rows, dtype=np.uint32)
        per_row = [np.zeros(0, np.uint32) if r == 0 else p.ops[r - 1] for p in parts for r in range(p.n_rows)]
        self.ops_ptr = np.zeros(self.n_rows + 1, dtype=np.uint64)
        np.cumsum([len(o) for o in per_row], out=self.ops_ptr[1:])
        self.ops = np.concatenate(per_row).astype(np.uint32)
        self.deg = np.concatenate([p.deg for p in parts])

    def single(self, i):
        """(row_ids, ops, ops_ptr) of partition i for isocon_msa_build_ops"""
        r0, r1 = int(self.first_row[i]), int(self.first_row[i + 1])
        o0 = int(self.ops_ptr[r0])
        return self.row_ids[r0:r1], self.ops[o0:int(self.ops_ptr[r1])], self.ops_ptr[r0:r1 + 1] - np.uint64(o0)


# ---- 3. the batched kernel's list limit -----------------------------------------------------------------------------------------------

def limit_partition(name, n_cand, rng, Lm=1200, n_quiet=6):
    """A member (row 1) that differs from the centre in its first n_cand positions -- by a substitution, or by a deletion at every seventh --
    a companion (row 2) that shares some of the substitutions (own count 2), and n_quiet members that each differ in one position of their
    own behind the noisy stretch (distinct sequences): the quiet rows and the centre hold every column's majority."""
    assert n_cand + n_quiet + 2 <= Lm
    c = random_seq(rng, Lm)
    noisy_row, t = [], 0
    while t < n_cand:
        if t % 7 == 3 and t + 1 < n_cand and t % 14 == 3:
            noisy_row.append(("D", t, 2))          # (a 2-base run now and then: two candidates)
            t += 2
        elif t % 7 == 3:
            noisy_row.append(("D", t, 1))
            t += 1
        else:
            noisy_row.append(("X", t))
            t += 1
    companion = [("X", t) for t in range(0, min(n_cand, 200), 5) if t % 7 != 3 and (t - 1) % 14 != 3]
    quiet = [[("X", n_cand + 1 + i)] for i in range(n_quiet)]
    return Partition(name, c, [noisy_row, companion] + quiet)


def limit_partitions():
    """ordinary partitions around one with a 1024-candidate row and one with a 1025-candidate row; all sequences distinct"""
    rng = np.random.default_rng(91)
    parts = []
    for i in range(5):
        c = random_seq(rng, 50 + i)
        parts.append(Partition("ordinary%d" % i, c, [_light_edits(rng, 50 + i) for _ in range(4)], degree=1 + (i % 2)))
    parts.insert(1, limit_partition("limit1024", 1024, rng))
    parts.insert(3, limit_partition("limit1025", 1025, rng))
    return parts
