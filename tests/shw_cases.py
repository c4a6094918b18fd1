"""Designed inputs for the prefix ("SHW") entries isocon_shw_locations / isocon_shw_path_pairs (csrc/shw.hpp, shw_host.inc) and the plain
restatement every test module compares with.  tests/test_shw_cases.py asserts on the CPU that every case sits where it claims (class,
round, end count) and ties the restatement to the oracle; tests/test_shw_core.py runs the cases through a tile emulator on
csrc/hw_core.hpp; tests/test_gpu_shw.py compares the device with the restatement on every pair.  Fixed seeds, standard library and numpy
only, no library load.

Construction as in tests/hw_edge_cases.py: query bodies over A, C, G, everything else T, so a copy with d planted edits in front of a T
flank has distance d (read off the restatement, never assumed).

A case = SCase(name, group, query, targets, ks, what, lanes): ks[i] None = unbounded; lanes[i] holds what target i must give -- h (the
unbounded distance), n_ends, ends, words (window words of the kernel the pair settles in: 2 thr + 1 diagonals), round (the round that
settles it, None: no round does), kernel (False: the lengths alone decide in every round)."""
import functools
import random
from collections import namedtuple

import numpy as np

import hw_edge_cases as E

SCase = namedtuple("SCase", "name group query targets ks what lanes")

CLASS_P = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)
CLASS_H = (0, 1, 31, 32, 63, 64, 127, 128, 255)
TILE_SIZES = (1, 63, 64, 65, 130)
ROUND_THR = (31, 63, 127, 255)

words = E.words
body, plant, rnd = E.body, E.plant, E.rnd


# ---- the restatement: the issue's DP, a row at a time --------------------------------------------------------------------------------
def last_row(q, t):
    """row len(q) of D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (q[i-1] != t[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)"""
    n = len(t)
    tt = np.frombuffer(t.encode(), dtype=np.uint8)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = ar.copy()
    for i, c in enumerate(q.encode(), 1):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (tt != c))
        prev = np.minimum.accumulate(cur - ar) + ar          # the insertion term D[i][j-1] + 1 along the row
    return prev


def restated(q, t, k):
    """(h or -1, [end, ...]): h = min over 1 <= j <= n of D[P][j], a hit iff h <= k (k None: always), the ends every 0-based j - 1 with
    D[P][j] == h, ascending; an empty q or t is a miss"""
    if len(q) == 0 or len(t) == 0:
        return -1, []
    last = last_row(q, t)[1:]
    h = int(last.min())
    if k is not None and h > k:
        return -1, []
    return h, np.nonzero(last == h)[0].tolist()


@functools.lru_cache(maxsize=None)
def restated_cached(q, t, k):
    h, ends = restated(q, t, k)
    return h, tuple(ends)


# ---- what the host driver does with a pair (csrc/shw_host.inc, restated) ----------------------------------------------------------------
def clamp(k, P):
    return P if k is None or k < 0 else min(k, P)


def needs_kernel(P, n, thr):
    return P > 0 and n > 0 and n - P >= -thr


def settles(P, n, k, h):
    """(round, threshold of that round) in which the pair leaves the distance stage -- it hits (h = its unbounded distance), or has missed
    at its own threshold --, (None, None) when no round settles it"""
    kc = clamp(k, P)
    for r, cap in enumerate(ROUND_THR):
        thr = min(kc, cap)
        if (needs_kernel(P, n, thr) and 0 <= h <= thr) or thr == kc:
            return r, thr
    return None, None


def _rng(*key):
    return random.Random("shw_cases/" + "/".join(str(x) for x in key))


def _lane(q, t, k, **claims):
    h, ends = restated_cached(q, t, None)
    r, thr = settles(len(q), len(t), k, h)
    return dict(claims, h=h, round=r, words=None if thr is None else words(2 * thr + 1))


# ---- a. class edges ------------------------------------------------------------------------------------------------------------------
def group_a():
    """every P with targets whose distance falls on the class edges: the body with d edits in front of a T flank (d <= P - 4), all T (d = P);
    each with k = h -- a hit exactly at the threshold -- and k = h - 1, a miss"""
    for P in CLASS_P:
        rng = _rng("a", P)
        b = body(rng, P)
        targets, ks, lanes = [], [], []
        for d in CLASS_H:
            if d == P:
                made = ["T" * (P + 7)]
            elif d <= P - 4:
                # (deletions and insertions only while they are sparse: dense ones realign more cheaply than planted)
                made = [plant(b, d, kind) + "T" * 9 for kind in (("sub", "del", "ins") if 0 < 4 * d <= P else ("sub",))]
            else:
                continue
            for t in made:
                h = restated_cached(b, t, None)[0]
                for k in ([h, h - 1] if h else [h]):
                    targets.append(t); ks.append(k)
                    lanes.append(_lane(b, t, k, planted=d, hit=k >= h))
        yield SCase("a_P%d" % P, "a", b, targets, ks, "query of %d bases, distances on the class edges, k = h and k = h - 1" % P, lanes)


# ---- b. length rule ------------------------------------------------------------------------------------------------------------------
def group_b():
    rng = _rng("b")
    b = body(rng, 40)
    P = len(b)
    for k in (0, 1, 5, 12):
        short = b[:P - k]          # reachable by k deletions only
        yield SCase("b_short_k%d" % k, "b", b, [short, short[:-1]], [k, k], "n = P - k (k query-only steps at the end) and n = P - k - 1: a miss without a kernel",
                    [_lane(b, short, k, h_is=k, ends=[P - k - 1]), _lane(b, short[:-1], k, kernel=False)])
    yield SCase("b_n1", "b", "ACG", ["A", "C", "T", "A"], [3, 2, None, 1], "a target of one base",
                [_lane("ACG", "A", 3, h_is=2, ends=[0]), _lane("ACG", "C", 2, h_is=2, ends=[0]), _lane("ACG", "T", None, h_is=3, ends=[0]), _lane("ACG", "A", 1, kernel=False)])
    p30 = body(rng, 30)
    long_t = plant(p30, 2, "sub") + rnd(rng, 3000 - 30)
    yield SCase("b_30_in_3000", "b", p30, [long_t, long_t], [5, None], "a 30-base query against a 3 000-base target: only its first P + k columns are read",
                [_lane(p30, long_t, 5, h_is=2), _lane(p30, long_t, None, h_is=2)])
    # ends at P + h - 1 (h target-only bases inside the copy) and P - h - 1 (h query-only)
    for h in (1, 3, 8):
        ins, dele = plant(b, h, "ins") + "T" * 20, plant(b, h, "del") + "T" * 20
        yield SCase("b_extremes_h%d" % h, "b", b, [ins, dele], [h, h], "ends at P + h - 1 and P - h - 1",
                    [_lane(b, ins, h, h_is=h, has_end=P + h - 1), _lane(b, dele, h, h_is=h, has_end=P - h - 1)])
    # the same targets cut to P + k bases give the same rows
    for k in (0, 2, 9):
        full = [plant(b, min(k, 2), "sub") + rnd(rng, 100), plant(b, k, "ins") + rnd(rng, 60), plant(b, k + 1, "sub") + rnd(rng, 60)]
        cut = [t[:P + k] for t in full]
        yield SCase("b_cut_k%d" % k, "b", b, full + cut, [k] * 6, "targets and the same cut to P + k bases: the same rows",
                    [_lane(b, t, k, same_as=(i + 3) % 6) for i, t in enumerate(full + cut)])


# ---- c. many ends --------------------------------------------------------------------------------------------------------------------
def group_c():
    yield SCase("c_a20", "c", "A" * 20, ["A" * 10 + "C" * 40], [10], "11 ends, h = 10", [_lane("A" * 20, "A" * 10 + "C" * 40, 10, h_is=10, ends=list(range(9, 20)))])
    for P, m in ((50, 20), (100, 64), (70, 69)):
        q, t = "A" * P, "A" * m + "C" * (2 * P)
        yield SCase("c_a%d_m%d" % (P, m), "c", q, [t, t], [P - m, None], "%d ends, h = %d" % (P - m + 1, P - m),
                    [_lane(q, t, P - m, h_is=P - m, ends=list(range(m - 1, P))), _lane(q, t, None, h_is=P - m, ends=list(range(m - 1, P)))])
    # ends that straddle columns 32 and 64
    for P in (28, 34) + tuple(range(60, 69)):
        q, t = "G" * P, "G" * (P - 5) + "T" * 40
        yield SCase("c_straddle_P%d" % P, "c", q, [t], [7], "6 ends P - 6 .. P - 1", [_lane(q, t, 7, h_is=5, ends=list(range(P - 6, P)))])
    yield SCase("c_acgtc", "c", "ACGTC", ["ACGTAC"], [2], "three ends", [_lane("ACGTC", "ACGTAC", 2, h_is=1, ends=[3, 4, 5])])


# ---- d. tiles ------------------------------------------------------------------------------------------------------------------------
def group_d():
    for n in TILE_SIZES:
        rng = _rng("d", n)
        b = body(rng, 45)
        targets, ks, lanes = [], [], []
        for i in range(n):
            d = i % 7
            t = plant(b, d, ("sub", "del", "ins")[i % 3]) + rnd(rng, (i * 13) % 90)
            k = i % 32          # per-pair thresholds 0 .. 31 mixed inside a tile
            targets.append(t); ks.append(k)
            lanes.append(_lane(b, t, k))
        yield SCase("d_targets%d" % n, "d", b, targets, ks, "%d targets of mixed lengths on one query, thresholds 0 .. 31" % n, lanes)
    # several queries in one call (three cases), one pair listed twice
    for j, P in enumerate((12, 33, 70)):
        rng = _rng("d", "multi", P)
        b = body(rng, P)
        targets = [plant(b, d, "sub") + rnd(rng, 10 * d) for d in range(0, 6)]
        targets.append(targets[2])
        ks = [3] * len(targets)
        yield SCase("d_multi%d" % j, "d", b, targets, ks, "query %d of three in one call; pair 2 listed twice" % j, [_lane(b, t, 3) for t in targets])


# ---- e. rounds -----------------------------------------------------------------------------------------------------------------------
def group_e():
    """P = 600, k = None: planted distances in (0, 31], (31, 63], (63, 127], (127, 255] settle in rounds 0 .. 3"""
    rng = _rng("e")
    b = body(rng, 600)
    targets = [plant(b, d, kind) + rnd(rng, 50) for d, kind in ((7, "sub"), (31, "del"), (40, "ins"), (63, "sub"), (100, "del"), (127, "sub"), (200, "ins"), (255, "sub"))]
    yield SCase("e_rounds", "e", b, targets, [None] * len(targets), "distances of every round under k = None",
                [_lane(b, t, None, in_round=r) for t, r in zip(targets, (0, 0, 1, 1, 2, 2, 3, 3))])


def far_pair():
    """(query, target) of group e's query with a distance above 255: no round settles it under k = None"""
    c, = cases("e")
    return c.query, plant(c.query, 300, "sub") + "T" * 20


@functools.lru_cache(maxsize=None)
def cases(group):
    return tuple({"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e}[group]())


ALL_GROUPS = tuple("abcde")


def flatten(case_list):
    """(seqs, q, t, k, owner) for one store: every query and target a sequence of its own, owner[p] = (case, lane); k[p] None = unbounded"""
    seqs, q, t, k, owner = E.flatten(case_list)
    return seqs, q, t, k, owner


def send_k(k):
    """thresholds as SeqStore takes them: -1 for None"""
    return [-1 if x is None else x for x in k]


@functools.lru_cache(maxsize=None)
def expected(group):
    """{(case name, lane): (h or -1, ends)} by the restatement, computed once per process (do not change it)"""
    return {(c.name, i): restated_cached(c.query, t, k) for c in cases(group) for i, (t, k) in enumerate(zip(c.targets, c.ks))}


def query_tiles(thrs, need):
    """tiles of one query's pairs as the builder forms them: pairs that need a kernel, by class of 2 thr + 1, runs of 64: {words: tiles}"""
    out = {}
    for w in (1, 2, 4, 8):
        c = sum(1 for thr, nd in zip(thrs, need) if nd and words(2 * thr + 1) == w)
        if c:
            out[w] = (c + 63) // 64
    return out


# ---- the random list ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_list(n_pairs=2000, seed=5):
    """(seqs, q, t, k): queries and targets of 1 .. 200 bases over ACGT; a target is a mutated copy of its query behind or in front of
    random bases, a cut copy, or random; k from a small set, None included"""
    rng = random.Random("shw_cases/random/%d" % seed)
    seqs, q, t, k = [], [], [], []
    while len(q) < n_pairs:
        P = rng.randint(1, 200)
        query = rnd(rng, P)
        qi = len(seqs)
        seqs.append(query)
        for _ in range(rng.randint(1, 40)):
            how = rng.random()
            if how < 0.6:
                c = list(query)
                for _ in range(rng.choice((0, 0, 1, 2, 3, 5, 8, 20, 60))):
                    i = rng.randrange(len(c)) if c else 0
                    if c:
                        c[i] = rng.choice(("", rng.choice("ACGT"), c[i] + rng.choice("ACGT")))
                tgt = "".join(c) + rnd(rng, rng.randint(0, 60))
            elif how < 0.75:
                tgt = query[:rng.randint(1, P)]
            else:
                tgt = rnd(rng, rng.randint(1, 200))
            tgt = (tgt or "A")[:200]
            q.append(qi)
            t.append(len(seqs))
            seqs.append(tgt)
            k.append(rng.choice((0, 1, 2, 5, 10, 31, 32, 70, None)))
    return tuple(seqs), tuple(q[:n_pairs]), tuple(t[:n_pairs]), tuple(k[:n_pairs])
