"""Inputs for the placement of wide-slot insertions (isocon_amd/csrc/msa_place_core.hpp, k_msa_slot_rep / k_msa_place of csrc/msa.hpp):
pairs (representative, insertion) with the step of functions.get_best_solution that places them -- tests/test_msa_place_core.py runs them
through the CPU emulator -- and partitions built around such pairs for tests/test_gpu_msa_place.py.  Fixed seeds, numpy only."""
from itertools import product

import numpy as np

import msa_cases as MC
from isocon_amd import functions as FUN

SUBSTRING, THREADED, OFFSET, LEFT = 0, 1, 2, 3
CAP = 62          # the longest insertion of a slot that the device places


def anchor(rep, q):
    """(columns of functions.get_best_solution("-" + rep + "-", q) as a str, the step that gave them)"""
    mx = "-" + rep + "-"
    cols = "".join(FUN.get_best_solution(mx, q))
    assert len(cols) == len(mx) and cols.replace("-", "") == q
    if mx.find(q) >= 0:
        return cols, SUBSTRING
    if FUN.min_ed(mx, q):
        return cols, THREADED
    return cols, (LEFT if cols.startswith(q) else OFFSET)


def exhaustive_pairs():
    """every representative of 2, 3 and 4 bases against every insertion of 1 base up to its own length"""
    out = []
    for n in (2, 3, 4):
        qs = ["".join(t) for m in range(1, n + 1) for t in product("ACGT", repeat=m)]
        for rep in product("ACGT", repeat=n):
            rep = "".join(rep)
            out.extend((rep, q) for q in qs)
    return out


def mutate(rng, s, n_edits):
    s = list(s)
    for _ in range(n_edits):
        kind = int(rng.integers(0, 3))
        at = int(rng.integers(0, max(len(s), 1)))
        if kind == 0 and s:
            s[at] = "ACGT"[int(rng.integers(0, 4))]
        elif kind == 1 and len(s) > 1:
            del s[at]
        elif kind == 2 and s:
            s[at] = s[at - 1]          # (repeats: ties in the backtrack)
    return "".join(s)


RANDOM_LONGEST = (5, 31, 32, 33, 61, 62)


def random_pairs(per_length=500, seed=5):
    """longest in RANDOM_LONGEST, m from 1 to longest; every second insertion a mutated copy (or a mutated piece) of the representative"""
    rng = np.random.default_rng(seed)
    out = []
    for n in RANDOM_LONGEST:
        for k in range(per_length):
            rep = MC.random_seq(rng, n)
            m = int(rng.integers(1, n + 1)) if k % 7 else (1, n)[(k // 7) % 2]
            if k % 2:
                a = int(rng.integers(0, n - m + 1))
                q = mutate(rng, rep[a:a + m], int(rng.integers(1, 4)))
                if not q:
                    q = "A"
            else:
                q = MC.random_seq(rng, m)
            assert 1 <= len(q) <= n
            out.append((rep, q))
    return out


def representative_sets(seed=9):
    """[(insertions of one slot, all equally long)]: sets that differ first at base 1, 32, 33 and 62 (1-based), and sets of equal strings"""
    rng = np.random.default_rng(seed)
    sets = []
    for n, first_diff in ((62, 1), (62, 32), (62, 33), (62, 62), (33, 33), (32, 32), (40, 1), (2, 2)):
        base = MC.random_seq(rng, n)
        d = first_diff - 1
        variants = [base[:d] + c + MC.random_seq(rng, n - d - 1) for c in "TGCA"]          # the smallest comes last
        extra = [base[:d] + "T" + MC.random_seq(rng, n - d - 1) for _ in range(3)]
        sets.append(variants + extra)
        sets.append(extra + variants[::-1])
    for n in (2, 32, 33, 62):
        s = MC.random_seq(rng, n)
        sets.append([s] * 5)
    # every string shares the first 32 bases: the second key alone decides
    head = MC.random_seq(rng, 32)
    sets.append([head + MC.random_seq(rng, 20) for _ in range(9)])
    # the smallest head comes with a large tail, a larger head with the smallest tail: the tail of another head must not win
    sets.append(["A" * 32 + "T" * 10, "A" * 31 + "C" + "A" * 10, "A" * 32 + "G" * 10])
    return sets


# ---- partitions for the device -----------------------------------------------------------------------------------------------------------

def find_pairs(n, outcome, count, seed=1):
    """`count` pairs (rep of n bases, q) that `outcome` places, from the exhaustive enumeration for n <= 4, else at random"""
    rng = np.random.default_rng(seed)
    out = []
    if n <= 4:
        for rep, q in exhaustive_pairs():
            if len(rep) == n and (len(q) < n or q > rep) and anchor(rep, q)[1] == outcome:          # (rep stays the slot's representative)
                out.append((rep, q))
        step = max(len(out) // count, 1)
        return out[::step][:count]
    while len(out) < count:
        rep = MC.random_seq(rng, n)
        m = int(rng.integers(1, n + 1))
        q = MC.random_seq(rng, m) if rng.random() < 0.5 else (mutate(rng, rep[:m], 2) or "A")
        if anchor(rep, q)[1] == outcome:
            out.append((rep, q))
    return out


def slot_members(slot, strings):
    """one member per string, each with that insertion in `slot`"""
    return [[("I", slot, s)] for s in strings]


def build_partitions():
    """{name: Partition}; every partition has at most 70 rows and a centre of at most 1 100 bases.  PLAN[name] = {slot: what is expected of
    it}: "placed" or "left"."""
    rng = np.random.default_rng(2024)
    P, plan = {}, {}

    def add(name, centre, member_edits, slots, degree=1):
        P[name] = MC.Partition(name, centre, member_edits, degree=degree)
        plan[name] = slots

    # the four outcomes, four pairs each from the enumeration: one slot per pair (the representative and the insertion alone in it; a third
    # row repeats the insertion, so the placement is written twice)
    edits, slots = [], {}
    c = MC.random_seq(rng, 200)
    t = 3
    outcome_pairs = []
    for outcome in (SUBSTRING, THREADED, OFFSET, LEFT):
        for rep, q in find_pairs(4, outcome, 4):
            outcome_pairs.append((t, rep, q, outcome))
            t += 11
    rows = [[], [], []]
    for t, rep, q, outcome in outcome_pairs:
        rows[0].append(("I", t, rep)); rows[1].append(("I", t, q)); rows[2].append(("I", t, q))
        slots[t] = "placed"
    add("outcomes", c, rows + [[("X", 7)]], slots, degree=2)
    P["outcomes"].outcome_pairs = outcome_pairs

    # longest 2, 3, 32, 33, 62 (placed) and 63, 64, 70 (left) in ONE partition, with m = 1 and m = longest in every slot; slot 0 and slot Lm
    c = MC.random_seq(rng, 300)
    longest_at = {0: 2, 20: 3, 50: 32, 90: 33, 130: 62, 170: 63, 210: 64, 250: 70, 300: 5}
    rows = [[] for _ in range(5)]
    for t, n in longest_at.items():
        rep = MC.random_seq(rng, n)
        rows[0].append(("I", t, rep))
        rows[1].append(("I", t, MC.random_seq(rng, n)))                     # m = longest, another string
        rows[2].append(("I", t, MC.random_seq(rng, 1)))                     # m = 1
        rows[3].append(("I", t, mutate(rng, rep[:n - 1], 2) or "C"))        # threads or falls to the offsets
        rows[4].append(("I", t, rep[1:n - 1] if n > 2 else "G"))            # a substring (n = 2: a single base)
    rows[1].append(("X", 100)); rows[2].append(("D", 110, 3))
    add("lengths", c, rows, {t: ("placed" if n <= CAP else "left") for t, n in longest_at.items()})

    # longest insertions that differ only behind base 32; and two that differ at base 62
    c = MC.random_seq(rng, 120)
    head = MC.random_seq(rng, 32)
    tails = ["TTGA" + MC.random_seq(rng, 6), "TTCA" + MC.random_seq(rng, 6), "TTCC" + MC.random_seq(rng, 6), "TTCA" + "A" * 6]
    long62 = MC.random_seq(rng, 61)
    rows = [[("I", 30, head + tl), ("I", 80, long62 + "TGCA"[i])] for i, tl in enumerate(tails)]
    rows.append([("I", 30, head[5:] + "AC"), ("I", 80, long62[10:50])])
    rows.append([("I", 30, mutate(rng, head + tails[1], 3)), ("I", 80, mutate(rng, long62, 3))])
    add("behind_base_32", c, rows, {30: "placed", 80: "placed"})

    # more than 64 rows with the same string in one slot, and more than 64 distinct strings in another
    c = MC.random_seq(rng, 90)
    distinct = sorted({MC.random_seq(rng, int(rng.integers(1, 7))) for _ in range(200)})[:67]
    assert len(distinct) == 67 and max(map(len, distinct)) >= 2
    rows = [[("I", 40, "ACCA"), ("I", 60, s)] for s in distinct]
    rows[0][0] = ("I", 40, "TACCAG")
    add("many_rows", c, rows + [[("I", 40, "GGGGGG")]], {40: "placed", 60: "placed"})

    # two partitions with a wide slot at the same t and different representatives
    c = MC.random_seq(rng, 70)
    add("twin_a", c, [[("I", 33, "ACGTAC")], [("I", 33, "GTT")], [("I", 33, "CGA")]], {33: "placed"})
    add("twin_b", c[:35] + "T" + c[35:], [[("I", 33, "TTTTGG")], [("I", 33, "GTT")], [("I", 33, "CGA")], [("I", 33, "TTTTGA")]], {33: "placed"}, degree=3)

    # no wide slot at all
    c = MC.random_seq(rng, 64)
    add("no_wide_slot", c, [[("I", 5, "A"), ("X", 9)], [("I", 5, "C"), ("D", 30, 2)], [("I", 64, "T")], []], {})

    # a row with more than 64 ops and wide insertions in both halves of its ops
    c = MC.random_seq(rng, 1100)
    many = MC.n_ops_member(c, 90)
    last = max(e[1] for e in many) + 5
    many = [("I", 0, "GATTACA")] + [e for e in many if not (e[0] == "I" and e[1] == 0)] + [("I", last, "CCGT"), ("I", 1100, "TGA")]
    add("many_ops", c, [many, [("I", 0, "GATT"), ("I", last, "CGT"), ("I", 1100, "GAT")], [("I", 0, "TTACAGG"), ("I", last, "AC")],
                        [("I", 2, "AG"), ("I", 1100, "TG")]], {0: "placed", 2: "placed", last: "placed", 1100: "placed"})
    return P, plan


ORDER = ["outcomes", "twin_a", "lengths", "no_wide_slot", "twin_b", "behind_base_32", "many_rows", "many_ops"]
