"""Designed inputs for the distance, bound, nearest-neighbour and alignment kernels (tests/test_gpu_planted_edges.py compares the device
with the oracle on them, tests/test_planted_cases.py asserts on the CPU that every input still has the property it was built for).
Fixed seeds, numpy only, no library load.

Planted pairs: y is x with d edits at positions `spacing` apart, so that the edit distance is a chosen number -- the last value a band
of 64 W rows holds (64 W - 1), the first it does not (64 W), and 31 / 32 for the 32-row form of the table kernel -- and not whatever a
random read happens to give.  Deletions and insertions alone make |len(x) - len(y)| = d: the distance is d by construction and the
optimal path ends on the extreme diagonal of a band of exactly d.  Edits spaced 8 bases and more apart make the two lower bounds of the
nearest-neighbour search (tests/qgram_ref.py) tight or nearly so.

Excursion pairs: s1 = P U M S against s2 = P M V S, with U, V random g-mers: the optimal semi-global alignment leaves the main diagonal by
g, stays there for |M| columns and comes back, and with match 2, open 2, ext 0 it scores 2 (|P| + |M| + |S|) - 4, so the certificate of
the banded kernels (csrc/sg_host.inc) holds exactly when the half-width X is at least g + 2."""
import functools
from collections import namedtuple

import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)

EDGES = (63, 64, 127, 128, 255, 256, 511, 512)          # the last distance of every rung of the band ladder and the first beyond it
TABLE_EDGES = (31, 32)                                   # ... of the 32-row form of the table kernel
KINDS = ("del", "ins", "sub", "mix")


def random_seq(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes().decode()


def plant(x, d, kind, spacing, seed):
    """x with d edits, one every `spacing` bases, the run of edits centred in x.  del: the base is left out; ins: a base in front of it;
    sub: another base; mix: insertions at the first ceil(d / 2) positions, deletions at the others (the path leaves the main diagonal by
    d / 2 and comes back; d odd leaves the result one base longer)."""
    L = len(x)
    assert kind in KINDS and d >= 0 and spacing >= 1 and (d == 0 or (d - 1) * spacing < L)
    rng = np.random.default_rng(seed)
    xs = np.frombuffer(x.encode(), dtype=np.uint8)
    first = (L - ((d - 1) * spacing + 1)) // 2 if d else 0
    at = {first + i * spacing: i for i in range(d)}
    new = rng.integers(0, 4, max(d, 1))
    step = rng.integers(1, 4, max(d, 1))
    out = []
    for t in range(L):
        i = at.get(t)
        if i is None:
            out.append(xs[t])
            continue
        what = kind if kind != "mix" else ("ins", "del")[i >= (d + 1) // 2]
        if what == "ins":
            out.append(BASES[new[i]])
            out.append(xs[t])
        elif what == "sub":
            out.append(BASES[(int(np.flatnonzero(BASES == xs[t])[0]) + step[i]) % 4])          # never the base itself
    return np.asarray(out, dtype=np.uint8).tobytes().decode()


def planted_pair(L, d, kind, spacing, seed):
    """(x, y): x random of length L, y = plant(x, ...)"""
    x = random_seq(np.random.default_rng(seed), L)
    return x, plant(x, d, kind, spacing, seed + 1000003)


Planted = namedtuple("Planted", "name x y d kind spacing")


def _case(L, d, kind, spacing, seed):
    x, y = planted_pair(L, d, kind, spacing, seed)
    return Planted("%s_d%d_s%d_L%d" % (kind, d, spacing, L), x, y, d, kind, spacing)


def _length(need, turn):
    """the smallest 64 j + (-1, 0, 1)[turn % 3] that holds `need` bases"""
    off = (-1, 0, 1)[turn % 3]
    return 64 * ((need - off + 63) // 64) + off


# seeds: SEED0 + running number.  The distance of a del / ins pair is d whatever the seed; a sub / mix pair whose sequences happen to
# allow a cheaper script would need another seed (tests/test_planted_cases.py requires the oracle's distance to be d for every pair)
SEED0 = 4100


def small_cases():
    """every d of TABLE_EDGES and 63, 64 x every kind x spacings 8, 9, 16; the pattern lengths take 64 j - 1, 64 j, 64 j + 1 in turn"""
    out, turn = [], 0
    for d in TABLE_EDGES + (63, 64):
        for spacing in (8, 9, 16):
            for kind in KINDS:
                L = _length((d - 1) * spacing + 1 + 2 * spacing, turn)
                out.append(_case(L, d, kind, spacing, SEED0 + turn))
                turn += 1
    return out


def large_cases():
    """127 .. 512 with the spacing that keeps x at about 1600 bases and less; y empty (L == d, deletions only)"""
    out, turn = [], 100
    for d, spacing in ((127, 8), (128, 8), (255, 5), (256, 5), (511, 3), (512, 3)):
        for kind in KINDS:
            L = _length((d - 1) * spacing + 1 + 16, turn)
            out.append(_case(L, d, kind, spacing, SEED0 + turn))
            turn += 1
    for d in (32, 63, 64, 128, 512):
        out.append(_case(d, d, "del", 1, SEED0 + turn))
        turn += 1
    return out


def planted_cases():
    return small_cases() + large_cases()


def full_pass_cases():
    """the un-banded kernel around its 4096 pattern rows per pass.  The kernel takes the SHORTER sequence as the pattern, so that is the
    one with the edge length: 4095, 4096 (one pass, its last row), 4097 (the first row of a second pass) and 8193 (of a third), each with
    a deletion partner (x has d bases more: the pattern is y), an insertion partner (the pattern is x) and a substitution partner, at
    distances 512 and 513 in turn (beyond every band)"""
    out = []
    i = 0
    for P in (4095, 4096, 4097, 8193):
        for kind in ("del", "ins", "sub"):
            d = 512 + i % 2
            out.append(_case(P + d if kind == "del" else P, d, kind, 7, 4300 + i))
            i += 1
    return out


def group_cases():
    """[(name, shared sequence, [(partner, d)])]: one sequence with 1, 15, 16, 64 and 65 planted partners (fewer than 16 pairs per shared
    sequence go one pair per lane, more into tiles of up to 64 lanes), and one whose 64 partners have every second length difference from
    -63 to +63: with k = d a lane's band runs from diagonal 0 to its length difference, so the lanes together need the 127 diagonals from
    -63 to +63 and no window of 64 holds them (how the library serves such a tile is not observable: the results are compared with the oracle)"""
    rng = np.random.default_rng(4400)
    out = []
    for n in (1, 15, 16, 64, 65):
        x = random_seq(rng, 703)
        partners = []
        for i in range(n):
            d = (63, 64, 31, 32, 62, 48, 17)[i % 7]
            kind = KINDS[i % 4]
            # the partners of one shared sequence: the same x, edits of their own (the spacing moves the positions)
            y = plant(x, d, kind, 8 + i % 3, 4500 + 100 * n + i)
            partners.append((y, kind, d))
        out.append(("group%d" % n, x, partners))
    x = random_seq(rng, 705)
    partners = []
    for i, diff in enumerate(range(-63, 64, 2)):
        kind = "del" if diff < 0 else "ins"
        partners.append((plant(x, abs(diff), kind, 9, 4900 + i), kind, abs(diff)))
    out.append(("spread", x, partners))
    return out


# ---- nearest-neighbour families ----------------------------------------------------------------------------------------------------

Family = namedtuple("Family", "d base members decoy")          # members: [(sequence, kind)] at exactly d; decoy at d + 1


def nn_families():
    """One family per d of TABLE_EDGES + EDGES: a base read, three members at exactly d (deletions or insertions in turn, substitutions,
    the mix) and a decoy at d + 1 (deletions / insertions, the other sign than the family's first member).  Bases are unrelated random
    sequences: about 700 bases for d <= 64, 1100 / 1350 / 1600 above."""
    out = []
    for i, d in enumerate(TABLE_EDGES + EDGES):
        L, spacing = {31: (700, 16), 32: (701, 16), 63: (703, 9), 64: (705, 9), 127: (1100, 8), 128: (1101, 8), 255: (1350, 5), 256: (1351, 5),
                      511: (1600, 3), 512: (1601, 3)}[d]
        rng = np.random.default_rng(5000 + i)
        base = random_seq(rng, L)
        first = ("del", "ins")[i % 2]
        members = [(plant(base, d, first, spacing, NN_SEEDS.get((d, first), 5100 + 10 * i)), first),
                   (plant(base, d, "sub", spacing, NN_SEEDS.get((d, "sub"), 5101 + 10 * i)), "sub"),
                   (plant(base, d, "mix", spacing, NN_SEEDS.get((d, "mix"), 5102 + 10 * i)), "mix")]
        other = ("ins", "del")[i % 2]
        decoy = plant(base, d + 1, other, spacing if (d + 1) * spacing < L else spacing - 1, 5103 + 10 * i)
        out.append(Family(d, base, members, decoy))
    return out


NN_SEEDS = {(511, "sub"): 5183}          # (d, kind) -> seed, where the default seed's member is not at exactly d (509: a cheaper script exists)


def nn_set():
    """(S: accession -> sequence, bases: {accession: d}) of all families"""
    S, bases = {}, {}
    for f in nn_families():
        S["base%d" % f.d] = f.base
        bases["base%d" % f.d] = f.d
        for s, kind in f.members:
            S["%s%d" % (kind, f.d)] = s
        S["decoy%d" % f.d] = f.decoy
    assert len(set(S.values())) == len(S) and len(S) < 100
    return S, bases


# ---- excursion pairs and band hints ---------------------------------------------------------------------------------------------------

FLANK, MIDDLE = 150, 400
MATCH = 2
GAP_MODELS = ((2, 0), (3, 0), (3, 1))
MISMATCHES = (-1, -2, -3, -4)
TARGET_DIAGS = (127, 128, 129, 255, 256, 257)


def excursion_pair(g, trim, seed):
    """(s1, s2) = (P U M S, P M V S) with |P| = |S| = FLANK, |M| = MIDDLE, U and V random g-mers; `trim` bases cut from the end of s2"""
    rng = np.random.default_rng(seed)
    P, U, M, V, S = (random_seq(rng, n) for n in (FLANK, g, MIDDLE, g, FLANK))
    s2 = P + M + V + S
    return P + U + M + S, s2[:len(s2) - trim]


def band_x(m, n, hint, mismatch, open_, ext, match=MATCH):
    """the half-width the alignment entry point derives from an edit-distance hint (restated in tests/test_gpu_planted_edges.py from
    csrc/sg_host.inc), or -1 where the pair is not banded"""
    aD = abs(n - m)
    Q = max(-mismatch, open_ + ext)
    X = max(((match + Q) * hint + match - 1) // match - aD + 1, 1)
    return X if aD + 2 * X + 64 < min(m, n) else -1


Hint = namedtuple("Hint", "hint mismatch open ext trim X")


@functools.lru_cache(maxsize=None)
def _hints(target_diags, model):
    """every (mismatch, trim, hint), in that order of loops, whose band |D| + 2 X + 1 on an excursion pair is target_diags wide under the gap
    model (the pair's lengths, 700 + g and 700 + g - trim, only decide whether it is banded at all: they are for every g >= 0)"""
    out = []
    m = 2 * FLANK + MIDDLE
    for mismatch in MISMATCHES:
        for trim in range(4):
            for hint in range(1, 200):
                X = band_x(m, m - trim, hint, mismatch, model[0], model[1])
                if X >= 0 and trim + 2 * X + 1 == target_diags:
                    out.append(Hint(hint, mismatch, model[0], model[1], trim, X))
    return out


def band_hint(target_diags, g, margin=None, models=GAP_MODELS):
    """the first (gap model, mismatch, trim, hint) whose band on the excursion pair (g, trim) is target_diags wide -- and, with `margin`,
    has X == g + margin.  None where there is none."""
    for model in models:
        for h in _hints(target_diags, model):
            if margin is None or h.X == g + margin:
                return h
    return None


EXCURSIONS_3_1 = ("diags127_open3_ext1_certifies", "diags128_open3_ext1_redone", "diags129_open3_ext1_certifies", "diags255_open3_ext1_redone")

Excursion = namedtuple("Excursion", "name s1 s2 g target hint certifies")


def gap_cost(g, open_, ext):
    return open_ + (g - 1) * ext


def excursion_cases():
    """For every target width two pairs under the gap model (2, 0): one with X == g + 2 (the path two diagonals inside the band's edge, the
    certificate just holds) and one with X == g + 1 (one diagonal inside, the certificate just fails); and the same two sides of the
    certificate under (3, 0) and (3, 1), where a gap of g bases costs 3 and 3 + (g - 1): X == g + cost and X == g + cost - 1.  Under (3, 1)
    X == 2 g + 2 or 2 g + 1 fixes the parity of X, and X = (target - 1 - trim) / 2 with trim < 4 allows few values: only the combinations
    of EXCURSIONS_3_1 exist (the targets 256 and 257 have none); (2, 0) and (3, 0) have both sides at every target."""
    out = []
    seed = 6000
    for target in TARGET_DIAGS:
        for model in GAP_MODELS:
            for certifies in (True, False):
                found = None
                for g in range(126, 3, -1):
                    h = band_hint(target, g, gap_cost(g, *model) - (0 if certifies else 1), models=(model,))
                    if h is not None:
                        found = (g, h)
                        break
                if found is None:
                    continue
                g, h = found
                s1, s2 = excursion_pair(g, h.trim, seed)
                seed += 1
                out.append(Excursion("diags%d_open%d_ext%d_%s" % (target, model[0], model[1], "certifies" if certifies else "redone"), s1, s2, g, target, h, certifies))
    return out
