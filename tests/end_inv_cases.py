"""Candidate sets of tests/test_end_inv_core.py (CPU, the core header under g++) and tests/test_gpu_end_invariant_graph.py (plain data makers,
no GPU): lengths and shifts around the 64-base words of the planes, one planted mismatch at either end of an overlap and either side of
every word boundary, runs of the padding's code past a sequence's end, periodic sequences whose first occurrence decides, equal sequences
and runs of equal lengths, sets under their own symbol map, and two random families.  expected_rows() is the reference's test,
end_invariant_functions._pair_is_invariant, over the reference's window, computed once per case."""
import bisect
import functools
import random

THRS = [0, 1, 15, 63, 64, 65, 130]
WORD_EDGE_LENGTHS = [63, 64, 65, 127, 128, 129, 191, 192, 193]


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def other(c):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[c]


def by_length(seqs):
    """the stable length sort of the product"""
    return sorted(seqs, key=len)


def window(lens, i, thr):
    return bisect.bisect_left(lens, lens[i] - 2 * thr), bisect.bisect_right(lens, lens[i])


@functools.lru_cache(maxsize=None)
def _expected(seqs, thr):
    from isocon_amd import end_invariant_functions as END
    lens = [len(s) for s in seqs]
    rows, pairs = [], 0
    for i, a in enumerate(seqs):
        lo, hi = window(lens, i, thr)
        pairs += hi - lo - 1
        rows.append([p for p in range(lo, hi) if p != i and END._pair_is_invariant(a, seqs[p], thr)])
    return rows, pairs


def expected_rows(seqs, thr):
    """(rows, window pairs) of a length-sorted list: row i = the positions p != i of i's window with _pair_is_invariant(seqs[i], seqs[p])"""
    return _expected(tuple(seqs), thr)


def partner(rng, A, n, d):
    """a sequence of length n that coincides with A on its whole overlap under the shift d (B[t] == A[t + d]), random outside A"""
    m = len(A)
    if d >= 0:
        body = A[d:d + n]
        return body + rnd(rng, n - len(body))
    return rnd(rng, -d) + A[:n + d]


# ---- lengths around the word edges -------------------------------------------------------------------------------------------------
def word_edge_lengths(thr):
    """A of each length around a word edge (for the wide thresholds also 256 and 320 bases further on, where every difference fits) with
    contained and overlapping partners at m - n in {0, 1, thr, thr + 1, 2 thr} and one at 2 thr + 1, just outside the window"""
    rng = random.Random(1000 + thr)
    lengths = list(WORD_EDGE_LENGTHS) + ([m + x for m in WORD_EDGE_LENGTHS for x in (256, 320)] if thr >= 63 else [])
    seqs = []
    for m in lengths:
        if m <= thr:
            continue
        A = rnd(rng, m)
        seqs.append(A)
        for diff in sorted({0, 1, thr, thr + 1, 2 * thr, 2 * thr + 1}):
            n = m - diff
            if n <= thr:
                continue
            shifts = {0, diff, diff // 2, min(diff, thr), diff + 1, thr, -1, diff - thr, (diff - thr) // 2}
            for d in sorted(shifts):
                if diff - thr <= d <= max(thr, diff) and n + min(d, 0) > 0 and m - d > 0:
                    seqs.append(partner(rng, A, n, d))
    return by_length(list(dict.fromkeys(seqs)))


# ---- one planted mismatch ----------------------------------------------------------------------------------------------------------
def planted_mismatches(thr):
    """Invariant partners of one A -- contained, suffix-prefix in either direction, at each extreme shift of the three ranges -- and, for each,
    copies with one base changed: the first and the last base of the overlap and either side of every word boundary of A's and of B's words.
    Returns (sorted list, A, the partners that are invariant without the mismatch, their mutated copies)."""
    from isocon_amd import end_invariant_functions as END
    rng = random.Random(2000 + thr)
    m = max(200, 3 * thr + 70)
    diff = thr // 2
    n = m - diff
    A = rnd(rng, m)
    shifts = [0, diff] + ([diff + 1, thr, diff - thr, -1] if thr > diff else [])
    good, bad = [], []
    for d in sorted(set(shifts)):
        B = partner(rng, A, n, d)
        assert END._pair_is_invariant(A, B, thr), (thr, d)
        good.append(B)
        t0, t1 = max(0, -d), min(n, m - d)          # the overlap in B's coordinates
        spots = {t0, t1 - 1}
        for t in range(t0, t1):
            if t % 64 in (0, 63) or (t + d) % 64 in (0, 63):
                spots.add(t)
        for t in sorted(spots):
            bad.append(B[:t] + other(B[t]) + B[t + 1:])
    return by_length(list(dict.fromkeys([A] + good + bad))), A, good, bad


# ---- bases past the end ------------------------------------------------------------------------------------------------------------
def past_the_end(thr):
    """The longer one is the shorter one's prefix plus a run of 'A' (code 0, the padding's code), also behind a sequence that ends in 'A's at
    a word boundary, and behind one that ends one base before it"""
    rng = random.Random(3000 + thr)
    base = max(100, 2 * thr + 40)
    S = rnd(rng, base - 1, "CGT") + "G"
    seqs = [S, S[:base - 10] + "A" * 10, S[:base - 10] + "A" * 20, S[:base - 1] + "A", S[:base - 1] + "AA"]
    for k in sorted({1, 2, thr, thr + 1, 2 * thr}):
        if k > 0:
            seqs.append(S + "A" * k)
            seqs.append(S[:base - 3] + "A" * (k + 3))
    for edge in (64, 128, 192):
        L = edge + (64 * ((thr + 63) // 64) if edge <= thr else 0)
        B = rnd(rng, L - 4, "CGT") + "AAAA"
        seqs += [B, B[:-1], B[:-4], B[:-5], "C" + B, "A" + B]
        for k in sorted({1, 2, 63, 64, thr, thr + 1, 2 * thr}):
            if 0 < k <= 2 * thr:
                seqs.append(B + "A" * k)
                seqs.append(B[:-4] + "A" * (k + 1))
    return by_length([s for s in dict.fromkeys(seqs) if len(s) > thr])


# ---- the first occurrence decides --------------------------------------------------------------------------------------------------
def first_occurrence(thr):
    """Periodic sequences (periods 2, 3 and 7) and their prefixes and phase-shifted cuts at many length differences: B occurs in A first at a
    shift that fails an end and again at one that would pass (no edge), and the mirrored case where the first occurrence passes"""
    m = max(150, 3 * thr + 40)
    seqs = []
    for unit in ("AC", "ACG", "ACGTTGA"):
        A = (unit * (m // len(unit) + 2))[:m]
        seqs.append(A)
        for diff in sorted({0, 1, 2, 3, 7, thr - 1, thr, thr + 1, thr + 2, thr + len(unit), 2 * thr - 1, 2 * thr}):
            if 0 <= diff <= 2 * thr:
                seqs.append(A[:m - diff])
                for s in (1, 2, 3):
                    if s <= diff:
                        seqs.append(A[s:s + m - diff])
    return by_length(list(dict.fromkeys(seqs)))


def first_occurrence_pair(thr):
    """(A, B that occurs first at shift 0 with m - n > thr left over and again at a shift that would pass, B2 whose first occurrence passes);
    None below thr 2 (no such pair)"""
    if thr < 2:
        return None
    m = max(150, 3 * thr + 40)
    m -= m % 2
    A = ("AC" * m)[:m]
    diff = thr + 2 if thr % 2 == 0 else thr + 1          # even, thr < diff <= 2 thr
    return A, A[:m - diff], A[:m - 2 * (thr // 2)]


# ---- equal sequences, runs of equal lengths ----------------------------------------------------------------------------------------
def equal_runs(thr):
    """Sequences that occur twice (two accessions of one sequence), runs of five and more equal lengths of related and unrelated sequences"""
    rng = random.Random(5000 + thr)
    L = max(130, 3 * thr + 30)
    A = rnd(rng, L)
    seqs = [A, A, A[1:] + "C", A[1:] + "C", "G" + A[:-1]]
    for _ in range(6):
        t = rng.randrange(L)
        seqs.append(A[:t] + other(A[t]) + A[t + 1:])
    for cut in (1, 2, min(thr, 9) + 1):
        seqs += [A[cut:], A[:-cut], A[cut:], rnd(rng, L - cut), rnd(rng, L - cut), A[:L - cut - 3] + rnd(rng, 3)]
    return by_length(seqs)


# ---- random families ---------------------------------------------------------------------------------------------------------------
def family_400(seed=1):
    """the 400-candidate generator of tests/test_end_invariants.py::test_anchor_index_finds_every_pair_the_quadratic_scan_finds: {acc: seq}"""
    rng = random.Random(seed)
    base = ["".join(rng.choice("ACGT") for _ in range(400 + rng.randint(-40, 40))) for _ in range(4)]
    C = {}
    for i in range(400):
        b = list(base[i % 4])
        for _ in range(rng.randint(0, 3)):
            b[rng.randrange(len(b))] = rng.choice("ACGT")
        b = "".join(b)
        r = rng.random()
        if r < 0.4:
            b = b[rng.randint(0, 25):len(b) - rng.randint(0, 25)]
        elif r < 0.6:
            b = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 20))) + b[rng.randint(0, 20):]
        elif r < 0.7:
            b = b[rng.randint(0, 20):] + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 20)))
        if b not in C.values():
            C["t_%d" % i] = b
    return C


def family_small(seed, thr, count=160, length=150):
    """three isoforms of about `length` bases, each candidate with up to two substitutions and ends trimmed or extended by up to thr + 3"""
    rng = random.Random(seed)
    base = [rnd(rng, length + rng.randint(-5, 5)) for _ in range(3)]
    out = []
    for i in range(count):
        b = list(base[i % 3])
        for _ in range(rng.choice((0, 0, 1, 2))):
            t = rng.randrange(len(b))
            b[t] = other(b[t])
        b = "".join(b)
        r = rng.random()
        if r < 0.5:
            b = b[rng.randint(0, thr + 3):len(b) - rng.randint(0, thr + 3)]
        elif r < 0.75:
            b = rnd(rng, rng.randint(0, thr + 3)) + b[rng.randint(0, thr + 3):]
        else:
            b = b[:len(b) - rng.randint(0, thr + 3)] + rnd(rng, rng.randint(0, thr + 3))
        out.append(b)
    return by_length(list(dict.fromkeys(out)))


RANDOM_FAMILIES = {
    "family_400_thr15": lambda: (by_length(list(family_400(1).values())), 15),
    "family_small_thr5": lambda: (family_small(7, 5), 5),
    "family_small_thr64": lambda: (family_small(8, 64, count=120, length=330), 64),
}


# ---- symbol maps -------------------------------------------------------------------------------------------------------------------
def own_map_sets():
    """(name, list, thr): a set in lower case and one over ACGU"""
    seqs = family_small(11, 15, count=60)
    return [("lower", [s.lower() for s in seqs], 15), ("acgu", [s.replace("T", "U") for s in seqs], 15)]


def directed_cases():
    """(name, length-sorted list, thr) of every directed case"""
    out = []
    for thr in THRS:
        out.append(("word_edge_lengths_thr%d" % thr, word_edge_lengths(thr), thr))
        out.append(("planted_mismatches_thr%d" % thr, planted_mismatches(thr)[0], thr))
        out.append(("past_the_end_thr%d" % thr, past_the_end(thr), thr))
        out.append(("first_occurrence_thr%d" % thr, first_occurrence(thr), thr))
        out.append(("equal_runs_thr%d" % thr, equal_runs(thr), thr))
    return out + own_map_sets()
