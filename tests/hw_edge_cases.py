"""Designed inputs for the banded infix kernels (isocon_hw_pairs: csrc/hw.hpp, hw_core.hpp, hw_tiles.hpp, hw_host.inc).
tests/test_hw_edge_cases.py asserts on the CPU that every input still has the property it was built for (and runs the set through the
tile emulator), tests/test_gpu_hw_edges.py compares the device with the oracle on every pair.  Fixed seeds, standard library only, no
library load; the oracle is loaded by oracle_rows() alone, the reference rows both test modules compare with.

A case = one query, its targets, one threshold per target and a claim: Case(name, group, query, targets, ks, what, lanes, tile), where
`what` says what the case is for, lanes[i] holds what target i must give (keys below) and `tile` what holds for the case as a whole.

How distances are made exact.  Query bodies are random over A, C, G; everything a target holds beside its copy of the body is T: flanks,
substituted bases, inserted bases.  A target made from a body with d bases deleted or replaced by T holds len(body) - d bases other than
T, so no infix matches more than that many query bases: the infix distance is at least d, and the copy attains it.  The same holds for a
query with bases the target lacks (a run of T in front of or behind the body: the overhangs of the leading / trailing insertion runs).
Inserted T (`ins`) cost one each as long as they lie inside the copy, two and more body bases apart.  With edits in the interior only,
the first end and the smallest start of the distance are those of the copy.  The CPU test holds every such statement against the oracle.

Lane claims: rows (diagonals of the pair's own LOCATE band), dist (the unbounded infix distance; a hit iff dist <= k), start, end, ms
(end - start + 1), lead, trail (insertion runs), ties ("ends" / "starts": at least two ends / two starts attain the distance), own_w
(window words of the pair's own LOCATE band), fin_w (words of its START / TRACE band, 2 k + 1 diagonals)."""
import functools
import random
from collections import namedtuple

HW_SEG = 8                       # csrc/hw_core.hpp

Case = namedtuple("Case", "name group query targets ks what lanes tile")

LOCATE_EDGES = (64, 65, 128, 129, 256, 257, 512)            # rows of the LOCATE band: the last of a class and the first of the next
FINISH_EDGES = (31, 32, 63, 64, 127, 128, 255)              # thresholds: 2 k + 1 = 63, 65, 127, 129, 255, 257, 511
BLOCK_ENDS = (30, 31, 32, 62, 63, 64, 65)                   # group d: `end` around the 32-column blocks and the 64-column text loads
BLOCK_TARGET_LENGTHS = (32, 33, 63, 64, 65, 127, 128, 129)
BLOCK_QUERY_LENGTHS = (63, 64, 65, 127, 128, 129)
HEAD_ENDS = (0, 1, 30, 31, 32, 33, 62, 63, 64)              # group f
RUNS = (1, 2, HW_SEG - 1, HW_SEG, HW_SEG + 1)               # group g, and the class's k
WINDOWS = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)              # group g: ms
FINISH_CLASS_K = (20, 50, 100, 200)                         # one threshold per finish class (41, 101, 201, 401 diagonals)
TILE_SIZES = (1, 2, 63, 64, 65, 130)                        # group h
PROMOTIONS = {1: ((40, 5), (0, 30)), 2: ((80, 10), (0, 60)), 4: ((200, 20), (0, 120))}      # W: two (delta, k) of W words, together 2 W


def rows(delta, k):
    """diagonals of the LOCATE band of a pair (csrc/hw_core.hpp hw_locate_rows)"""
    return max(delta, 0) + 2 * k + 1


def words(r):
    """window words of a band of r diagonals (csrc/hw_core.hpp hwt_words), 0: none"""
    return 1 if r <= 64 else 2 if r <= 128 else 4 if r <= 256 else 8 if r <= 512 else 0


def finish_grid_cap(W):
    """csrc/hw_plan.hpp hw_finish_grid_cap: the most workgroups a START / TRACE launch gets"""
    lds = HW_SEG * 2 * W * 64 * 8 if W == 2 else 0
    return 256 * (160 * 1024 // (lds + 256)) if W == 2 else 4096


def body(rng, n):
    """random over A, C, G; no base repeats its neighbour within the first and the last four, so that a copy shifted by a base against
    a flank costs more than the copy (an edit next to an end could otherwise move into the flank)"""
    out = []
    for i in range(n):
        c = rng.choice("ACG")
        while out and (i < 4 or i >= n - 4) and c == out[-1]:
            c = rng.choice("ACG")
        out.append(c)
    return "".join(out)


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def plant(b, d, kind):
    """b with d edits at evenly spaced interior positions: del (base left out), sub (T in its place), ins (T in front of it)"""
    assert kind in ("del", "sub", "ins") and (d == 0 or len(b) - 4 >= d)
    at = {2 + (i * (len(b) - 4)) // d for i in range(d)}
    assert len(at) == d
    out = []
    for i, c in enumerate(b):
        if i in at:
            if kind == "sub":
                out.append("T")
            elif kind == "ins":
                out.append("T" + c)
        else:
            out.append(c)
    return "".join(out)


def _rng(*key):
    return random.Random("hw_edge_cases/" + "/".join(str(x) for x in key))


# ---- a. LOCATE class edges ---------------------------------------------------------------------------------------------------
def group_a():
    """rows = 64 ... 512 reached mostly by k and mostly by delta.  Three targets per case, all P + delta long and all with the rows of the
    case: the body with k deletions behind delta + k bases of T (the path starts on the highest diagonal of the band and ends in the
    last column), the same in front of them (it ends on the lowest diagonal), and the body with k + 1 deletions: distance k + 1."""
    for R in LOCATE_EDGES:
        for how, k in (("k", (R - 1) // 2), ("delta", 5)):
            delta = R - 2 * k - 1
            rng = _rng("a", R, how)
            q = body(rng, max(40, 3 * k + 7))
            hit, miss = plant(q, k, "del"), plant(q, k + 1, "del")
            P = len(q)
            lanes = [dict(rows=R, dist=k, start=delta + k, end=P + delta - 1, lead=0, trail=0),
                     dict(rows=R, dist=k, start=0, end=P - k - 1, lead=0, trail=0),
                     dict(rows=R, dist=k + 1)]
            yield Case("a_rows%d_by_%s" % (R, how), "a", q, ["T" * (delta + k) + hit, hit + "T" * (delta + k), "T" * (delta + k + 1) + miss], [k] * 3,
                       "LOCATE band of %d diagonals (k %d, delta %d): hits on its highest and lowest diagonal, a near-miss" % (R, k, delta), lanes, {})


# ---- b. FINISH class edges ----------------------------------------------------------------------------------------------------
def group_b():
    """distance exactly k, all of it on one side: k deletions (the target is the shorter one, the path ends on diagonal -k) or, where
    3 k + 1 diagonals still fit 512, k insertions (it ends on diagonal +k)"""
    for k in FINISH_EDGES:
        rng = _rng("b", k)
        q = body(rng, 3 * k + 10)
        P = len(q)
        targets, lanes = [plant(q, k, "del")], [dict(dist=k, start=0, end=P - k - 1, ms=P - k, lead=0, trail=0, fin_w=words(2 * k + 1))]
        if rows(k, k) <= 512:
            targets.append(plant(q, k, "ins"))
            lanes.append(dict(dist=k, start=0, end=P + k - 1, ms=P + k, lead=0, trail=0, fin_w=words(2 * k + 1)))
        yield Case("b_k%d" % k, "b", q, targets, [k] * len(targets), "START / TRACE band of 2 x %d + 1 diagonals, the path on its outermost diagonal" % k, lanes, {})


# ---- c. length rules -----------------------------------------------------------------------------------------------------------
def group_c():
    rng = _rng("c")
    b = body(rng, 40)
    k = 10
    for lead, trail in ((k, 0), (0, k), (4, 6)):
        yield Case("c_overhang_%d_%d" % (lead, trail), "c", "T" * lead + b + "T" * trail, [b, b[:-1]], [k, k],
                   "delta = -k: the only hit is all overhang; delta = -k - 1: no kernel",
                   [dict(dist=k, start=0, end=39, lead=lead, trail=trail), dict(dist=k + 1)], {})
    for P, k in ((5, 5), (3, 8), (8, 8)):
        q = body(rng, P)
        targets = [rnd(rng, 20), "T" * 9, q, "T" * 3 + q[1:] + "T" * 40, q[:1]]
        yield Case("c_P%d_k%d" % (P, k), "c", q, targets, [k] * len(targets), "P <= k: every column is examined (jx = 1) and every target is a hit",
                   [dict(), dict(dist=P, start=0, end=0), dict(dist=0, start=0, end=P - 1), dict(dist=1), dict(dist=P - 1, start=0, end=0)], {})
    yield Case("c_P1", "c", "A", ["CCCA", "A", "GGG", "GGG", "AAAA"], [0, 0, 0, 1, 1], "P = 1",
               [dict(dist=0, start=3, end=3), dict(dist=0, start=0, end=0), dict(dist=1), dict(dist=1, start=0, end=0), dict(dist=0, start=0, end=0)], {})
    q = body(rng, 30)
    yield Case("c_k0", "c", q, [q + "T" * 10, "T" * 10 + q, q, "T" + q + "T", plant(q, 1, "sub")], [0] * 5, "k = 0: exact infix at the first and the last position",
               [dict(dist=0, start=0, end=29), dict(dist=0, start=10, end=39), dict(dist=0, start=0, end=29), dict(dist=0, start=1, end=30), dict(dist=1)], {})


# ---- d. column blocks of LOCATE -------------------------------------------------------------------------------------------------
def group_d():
    """`end` on both sides of every 32-column block edge, in the last column and in the first column examined (P - k - 1), for target
    lengths around the blocks (short queries) and for query lengths around the blocks"""
    k = 2
    for m in BLOCK_TARGET_LENGTHS:
        rng = _rng("d", "m", m)
        q = body(rng, 16)
        core = plant(q, 1, "sub")
        ends = sorted({e for e in BLOCK_ENDS + (m - 1, 15) if 15 <= e < m})
        targets = ["T" * (e - 15) + core + "T" * (m - 1 - e) for e in ends]
        yield Case("d_m%d" % m, "d", q, targets, [k] * len(ends), "targets of %d bases, the hit's end at %s" % (m, ends),
                   [dict(dist=1, start=e - 15, end=e, lead=0, trail=0) for e in ends], dict(longest=m))
    k = 3
    for P in BLOCK_QUERY_LENGTHS:
        rng = _rng("d", "P", P)
        q = body(rng, P)
        short, core = plant(q, k, "del"), plant(q, k, "sub")
        targets = [short + "T" * 9, "T" * 9 + short, "T" * 5 + core, core]
        lanes = [dict(dist=k, start=0, end=P - k - 1), dict(dist=k, start=9, end=P + 5), dict(dist=k, start=5, end=P + 4), dict(dist=k, start=0, end=P - 1)]
        for e in BLOCK_ENDS:
            if e >= P - 1 and e - P + 1 <= 9:
                targets.append("T" * (e - P + 1) + core + "T" * 4)
                lanes.append(dict(dist=k, start=e - P + 1, end=e))
        yield Case("d_P%d" % P, "d", q, targets, [k] * len(targets), "query of %d bases: end in the first column examined, in the last column, at block edges" % P, lanes, {})


# ---- e. tie rules -----------------------------------------------------------------------------------------------------------------
def group_e():
    rng = _rng("e")
    q = body(rng, 30)
    near = plant(q, 1, "sub")
    k = 3
    yield Case("e_copies", "e", q, ["T" * 5 + q + "T" * 7 + q + "T" * 3, "T" * 5 + q + "T" * 7 + q + "T" * 3 + q + "TT", "T" * 4 + near + "T" * 6 + q + "T" * 3,
                                   "T" * 4 + near + "T" * 6 + near + "T" * 3], [k] * 4, "two and three exact copies: the first end; a copy with one substitution in front of an exact one: the better one",
               [dict(dist=0, start=5, end=34, ties="ends"), dict(dist=0, start=5, end=34, ties="ends"), dict(dist=0, start=40, end=69), dict(dist=1, start=4, end=33, ties="ends")], {})
    # a query base the target lacks in front of a repeat the target has more of: inserting the base and substituting it cost the same
    b = body(rng, 24)
    for name, unit in (("homopolymer", "A"), ("dinucleotide", "AC"), ("trinucleotide", "GAC")):
        rep = (unit * 8)[:8]
        head = {"A": "C", "C": "G", "G": "A"}[rep[-5]]          # differs from the repeat base it is aligned with in the substitution
        q2 = head + rep[-4:] + b
        yield Case("e_starts_%s" % name, "e", q2, [rep + b + "TTT", "TT" + rep + b, rep + rep + b], [k] * 3,
                   "%s flank: several starts of the same distance, the smallest one" % name,
                   [dict(dist=1, ties="starts"), dict(dist=1, ties="starts"), dict(dist=1, ties="starts")], {})


# ---- f. START pass near the target's head -----------------------------------------------------------------------------------------
def group_f():
    """one query, so one tile: ends from 0 to 64 -- the reversed text of the START pass begins before the target (p0 < 0, p0 <= -32) or
    inside it, and min(end + 1, P + kmax) takes both branches"""
    rng = _rng("f")
    P = 20
    q = body(rng, P)
    core = plant(q, 2, "sub")
    targets, ks, lanes = [], [], []
    for e in HEAD_ENDS:                                   # (all targets 70 long and every pair's own band two words: one LOCATE tile)
        if e < P - 1:                                     # the first e + 1 query bases and nothing else that matches
            targets.append(q[:e + 1] + "T" * (69 - e))
            ks.append(P - 1)
            lanes.append(dict(dist=P - 1 - e, start=0, end=e, lead=0, trail=P - 1 - e, own_w=2))
        else:
            targets.append("T" * (e + 1 - P) + core + "T" * (69 - e))
            ks.append(8)
            lanes.append(dict(dist=2, start=e + 1 - P, end=e, lead=0, trail=0, own_w=2))
    yield Case("f_head_P20", "f", q, targets, ks, "ends %s in one tile, kmax = P - 1" % (HEAD_ENDS,), lanes, dict(kmax=P - 1, W=2))
    P, k = 33, 3
    q = body(rng, P)
    core = plant(q, 1, "sub")
    targets, lanes = [], []
    for e in HEAD_ENDS:
        if e < P - k - 1:
            continue
        if e < P - 1:
            targets.append(plant(q, P - 1 - e, "del") + "T" * 7)
            lanes.append(dict(dist=P - 1 - e, start=0, end=e))
        else:
            targets.append("T" * (e + 1 - P) + core + "TT")
            lanes.append(dict(dist=1, start=e + 1 - P, end=e))
    yield Case("f_head_P33", "f", q, targets, [k] * len(targets), "ends 30 ... 64 around a query of 33 bases", lanes, dict(kmax=k, W=1))


# ---- g. TRACE, checkpoints and the walk -------------------------------------------------------------------------------------------
def group_g():
    """per finish class (k = 20, 50, 100, 200).  The overhangs are runs of T, which the targets do not hold: a query T^r + body against the
    body starts with r insertions and start == 0; body + T^r against T + body ends with r and start == 1 (no leading run)."""
    for k in FINISH_CLASS_K:
        rng = _rng("g", k)
        fin_w = words(2 * k + 1)
        for r in RUNS + (k,):
            b = body(rng, 70)
            # edits on the path: a deletion / an insertion inside the first segment, on column 8, on column 16
            edits = [b[:3] + b[4:], b[:3] + "T" + b[3:], b[:7] + b[8:], b[:7] + "T" + b[7:], b[:15] + "T" + b[15:], b[:16] + b[17:]] if r + 1 <= k else []
            yield Case("g_k%d_lead%d" % (k, r), "g", "T" * r + b, [b] + edits, [k] * (1 + len(edits)), "leading run of %d, start == 0; edits in the first segments" % r,
                       [dict(dist=r, start=0, end=69, ms=70, lead=r, trail=0, fin_w=fin_w)] + [dict(dist=r + 1, start=0, lead=r, trail=0) for _ in edits], {})
            yield Case("g_k%d_trail%d" % (k, r), "g", b + "T" * r, [b, "T" + b, "TTT" + b] + edits[:2], [k] * (3 + len(edits[:2])), "trailing run of %d; start == 0, 1 and 3" % r,
                       [dict(dist=r, start=s, end=69 + s, ms=70, lead=0, trail=r, fin_w=fin_w) for s in (0, 1, 3)] + [dict(dist=r + 1, start=0, lead=0, trail=r) for _ in edits[:2]], {})
        for r, s in ((1, HW_SEG), (HW_SEG, 1), (HW_SEG + 1, 2), (k - HW_SEG + 1, HW_SEG - 1)):
            b = body(rng, 70)
            yield Case("g_k%d_both_%d_%d" % (k, r, s), "g", "T" * r + b + "T" * s, [b], [k], "both runs in one pair", [dict(dist=r + s, start=0, end=69, ms=70, lead=r, trail=s, fin_w=fin_w)], {})
        for ms in WINDOWS:
            b = body(rng, ms)
            targets, lanes = [b], [dict(dist=2, start=0, end=ms - 1, ms=ms, lead=2, trail=0, fin_w=fin_w)]
            if ms >= 7:                                   # the same window one column longer and one shorter, in the same tile
                targets += [b[:3] + "T" + b[3:], b[:3] + b[4:]]
                lanes += [dict(dist=3, start=0, ms=ms + 1, lead=2), dict(dist=3, start=0, ms=ms - 1, lead=2)]
            yield Case("g_k%d_ms%d" % (k, ms), "g", "TT" + b, targets, [k] * len(targets), "window of %d columns, start == 0, leading run of 2" % ms, lanes, {})
            flank = "T" if ms > 1 else {"A": "C", "C": "G", "G": "A"}[b]          # (a window of one base: T in front of it would match the overhang as well)
            yield Case("g_k%d_ms%d_start1" % (k, ms), "g", b + "TT", [flank + b], [k], "the mirror: start == 1, no leading run",
                       [dict(dist=2, start=1, end=ms, ms=ms, lead=0, trail=2, fin_w=fin_w)], {})


# ---- h. heterogeneous tiles ---------------------------------------------------------------------------------------------------------
def group_h():
    """one query against 1 ... 130 targets that share tiles: thresholds from 0 to the class cap, target lengths from P - k to P + delta_max,
    hits, near-misses, unrelated targets, a match behind unrelated bases, start == 0 lanes with windows from 8 columns to the whole target"""
    for W, blen, kmin, kcap, dmax, sizes in ((1, 34, 0, 28, 7, TILE_SIZES), (2, 120, 32, 50, 27, (64,)), (4, 250, 64, 100, 55, (2, 65))):
        assert rows(dmax, kcap) == 64 * W and words(rows(0, kmin)) == W          # (every pair of the class on its own, all of them together too)
        for n in sizes:
            rng = _rng("h", W, n)
            b = body(rng, blen)
            q = "TT" + b
            P = len(q)
            targets, ks = [], []
            for i in range(n):
                kind = i % 8
                k = kcap if i % 3 == 0 else rng.randint(kmin, kcap)
                if kind == 0:                              # start == 0, a window of 8 columns to the whole body, the rest a trailing run
                    k = kcap
                    ms = max(blen - (i // 8) * max(3, (blen - 8) // 7) % (blen - 7), P - k, 8)
                    t = b[:ms]
                elif kind == 1:                            # a hit with flanks
                    d = rng.randint(0, min(k, blen // 3))
                    a = rng.randint(0, dmax)
                    t = "T" * rng.randint(0, a) + plant(b, d, "sub")
                    t += "T" * rng.randint(0, max(0, P + a - len(t) - 2))
                elif kind == 2:                            # a near-miss: the body with k - 1 edits (+ 2 for the overhang)
                    t = plant(b, max(k - 1, 1), "sub" if k <= blen // 3 else "del") + "T" * rng.randint(0, 3)
                elif kind == 3:                            # unrelated, a small threshold: abandoned early
                    k = kmin + rng.randint(0, 4)
                    t = rnd(rng, rng.randint(max(1, P - k), P + dmax))
                elif kind == 4:                            # the only match in the last columns, behind unrelated bases
                    t = rnd(rng, dmax - 2) + plant(b, min(k, 2), "sub")
                elif kind == 5:                            # the shortest target the length rule lets through, and one base less (no kernel)
                    t = b[:max(1, P - k - (i // 8) % 2)]
                elif kind == 6:                            # the longest target of the class
                    t = "T" * (dmax + 2 - 5) + plant(b, min(k, 3), "ins" if k >= 3 else "sub")
                    t = t[:P + dmax] if len(t) > P + dmax else t + "T" * (P + dmax - len(t))
                else:                                      # the exact body somewhere, every other time with the smallest k (0: a miss by the overhang)
                    k = kmin if (i // 8) % 2 == 0 else k
                    a = rng.randint(0, dmax)
                    t = "T" * a + b + "T" * rng.randint(0, dmax - a)
                assert 1 <= len(t) <= P + dmax, (kind, len(t))
                targets.append(t)
                ks.append(k)
            yield Case("h_w%d_n%d" % (W, n), "h", q, targets, ks, "%d targets of one query in tiles of the class of %d words" % (n, W), [dict() for _ in targets],
                       dict(n=n, W=W, kmin=kmin, kcap=kcap, dmax=dmax))


def group_h_k_spread():
    """lane 0 has the smallest threshold of its tile and another lane's only end lies in the last column before P - k of lane 0: the first
    column examined is P - kmax of the tile, and the 32-column blocks before it are the unrolled ones"""
    rng = _rng("h", "k_spread")
    b = body(rng, 100)
    targets = [b, b[:70], b[:71], b[:85] + "TTT", plant(b, 2, "sub"), "T" * 4 + b[:96]]
    ks = [2, 30, 30, 15, 2, 30]
    lanes = [dict(dist=0, start=0, end=99), dict(dist=30, start=0, end=69, trail=30), dict(dist=29, start=0, end=70, trail=29), dict(dist=15, start=0, end=84, trail=15),
             dict(dist=2, start=0, end=99), dict(dist=4, start=4, end=99, trail=4)]
    yield Case("h_k_spread", "h", b, targets, ks, "k = 2 in lane 0, k = 30 and the end in column P - 30 in lane 1", lanes, dict(n=len(targets), W=1))


# ---- i. promotion --------------------------------------------------------------------------------------------------------------------
def group_i():
    """one query whose pairs need W words each and 2 W together: the device's buckets of (query, own class) put them into one tile, which
    is filed under 2 W; the host's greedy cut separates them"""
    for W, ((d1, k1), (d2, k2)) in sorted(PROMOTIONS.items()):
        rng = _rng("i", W)
        q = body(rng, max(100, 3 * k2 + 10))
        targets, ks, lanes = [], [], []
        for rep in range(2):
            for delta, k in ((d1, k1), (d2, k2)):
                a = (delta // 2, delta)[rep]
                targets.append("T" * a + plant(q, k - rep, "sub") + "T" * (delta - a))
                ks.append(k)
                lanes.append(dict(dist=k - rep, start=a, end=a + len(q) - 1, own_w=W, rows=rows(delta, k)))
        yield Case("i_w%d_to_w%d" % (W, 2 * W), "i", q, targets, ks, "pairs of %d words whose common window needs %d" % (W, 2 * W), lanes, dict(own_w=W, common_w=2 * W))


# ---- j. more tiles than the finish grid -------------------------------------------------------------------------------------------------
def group_j(W):
    """cap + 200 distinct queries with one target each, a start == 0 hit with a leading run: a workgroup's second tile differs from its
    first in the run, in ms and in the number of segments"""
    cap = finish_grid_cap(W)
    k, lo, hi = ((5, 24, 40), (40, 70, 90))[W - 1]
    rng = _rng("j", W)
    seen = set()
    for i in range(cap + 200):
        r = 1 + i % k
        ms = lo - r + (i * 7) % (hi - lo + 1)
        while True:
            b = body(rng, ms)
            if b not in seen:
                break
        seen.add(b)
        yield Case("j_w%d_%d" % (W, i), "j", "T" * r + b, [b], [k], "tile %d of %d, grid cap %d" % (i, cap + 200, cap), [dict(dist=r, start=0, end=ms - 1, ms=ms, lead=r, trail=0, fin_w=W)], dict(W=W, cap=cap))


@functools.lru_cache(maxsize=None)
def cases(group):
    """the cases of a group ("a" ... "i", "j1", "j2") as a tuple"""
    if group in ("j1", "j2"):
        return tuple(group_j(int(group[1])))
    made = tuple({"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e, "f": group_f, "g": group_g, "h": group_h, "i": group_i}[group]())
    return made + tuple(group_h_k_spread()) if group == "h" else made


ALL_GROUPS = tuple("abcdefghi") + ("j1", "j2")


MISS = [-1, -1, -1, 0, 0]


def oracle_row(x, y, k):
    """the five values isocon_hw_pairs returns for a pair, from the oracle's full matrices (hw_locate + nw_path)"""
    from oracle import oracle as O
    ed, start, end = O.hw_locate(x, y, k)
    if ed < 0:
        return list(MISS)
    _, ops = O.nw_path(x, y[start:end + 1])
    return [ed, start, end, ops[0][0] if ops[0][1] == "I" else 0, ops[-1][0] if ops[-1][1] == "I" else 0]


@functools.lru_cache(maxsize=None)
def oracle_rows(group):
    """{(case name, lane): row} of a group, computed once per process and shared by the tests (do not change it)"""
    return {(c.name, i): oracle_row(c.query, t, k) for c in cases(group) for i, (t, k) in enumerate(zip(c.targets, c.ks))}


def flatten(case_list, bystander=None):
    """(seqs, q, t, k, owner) of a list of cases for one store: every query and target a sequence of its own, owner[p] = (case, lane).
    bystander: a sequence appended behind all others (a longer one: the designed targets are not the last words of the planes)."""
    seqs, q, t, k, owner = [], [], [], [], []
    for c in case_list:
        qi = len(seqs)
        seqs.append(c.query)
        for lane, (target, kk) in enumerate(zip(c.targets, c.ks)):
            q.append(qi)
            t.append(len(seqs))
            seqs.append(target)
            k.append(kk)
            owner.append((c, lane))
    if bystander is not None:
        seqs.append(bystander)
    return seqs, q, t, k, owner


def host_tiles(case):
    """The LOCATE tiles the host's greedy cut forms for the pairs of one query (csrc/hw_plan.hpp hw_build_tiles with HwLocateCut, restated): a list of
    (W, [lanes]).  Pairs that need no kernel are in no tile."""
    P = len(case.query)
    need = [i for i, (t, k) in enumerate(zip(case.targets, case.ks)) if len(t) - P >= -k and P and len(t)]
    tiles = []
    for W in (1, 2, 4, 8):
        cur, dmax, kmax = None, 0, 0
        for i in need:
            delta, k = len(case.targets[i]) - P, case.ks[i]
            if words(rows(delta, k)) != W:
                continue
            d2, k2 = max(dmax, delta), max(kmax, k)
            if cur is not None and len(cur) < 64 and rows(d2, k2) <= 64 * W:
                cur.append(i)
                dmax, kmax = d2, k2
            else:
                cur = [i]
                tiles.append((W, cur))
                dmax, kmax = delta, k
    return tiles
