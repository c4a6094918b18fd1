"""Designed inputs for isocon_hw_locations (csrc/hw_loc.hpp, hw_loc_host.inc: every best location of an infix pair) and the plain
restatement both test modules compare with.  tests/test_hw_locations_cases.py asserts on the CPU that every claim of every case holds
under the restatement and ties the restatement to the oracle; tests/test_hw_locations_core.py runs the cases through a tile emulator
on csrc/hw_core.hpp; tests/test_gpu_hw_locations.py compares the device with the restatement on every pair.  Fixed seeds, standard
library and numpy only, no library load.

Construction as in tests/hw_edge_cases.py: query bodies over A, C, G, everything else T, so a planted copy with d edits has distance
exactly d and several copies in one target make several ends.

A case = LCase(name, group, query, targets, ks, what, lanes): lanes[i] holds what target i must give -- dist (the unbounded distance),
first ((start, end) of the first location), ends (all ends), n_ends, locs (all locations), ends_w / starts_w (window words of the pair's
ENDS band max(delta, 0) + 2 h + 1 and START band 2 h + 1), locate_w (of its LOCATE band, by k)."""
import functools
import random
from collections import namedtuple

import numpy as np

import hw_edge_cases as E

LCase = namedtuple("LCase", "name group query targets ks what lanes")

ENDS_EDGES = (64, 65, 128, 129, 256, 257, 512)         # diagonals of the ENDS band
START_EDGES = (31, 32, 63, 64, 127, 128)               # distances: 2 h + 1 = 63, 65, 127, 129, 255, 257
BLOCK_ENDS = (30, 31, 32, 33, 62, 63, 64, 65)          # the 32-column blocks and the 64-column text loads
TILE_SIZES = (1, 63, 64, 65, 130)
COPIES = (1, 2, 5)


# ---- the restatement: cell by cell, a row at a time ------------------------------------------------------------------------------
def _last_row(q, t, zero_top):
    """row len(q) of the edit-distance matrix of q (rows) against t (columns); zero_top: row 0 all zeros (infix), else row 0 = j"""
    n = len(t)
    tt = np.frombuffer(t.encode(), dtype=np.uint8)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, dtype=np.int64) if zero_top else ar.copy()
    for i, c in enumerate(q.encode(), 1):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (tt != c))
        # cur[j] = min(cur[j], cur[j - 1] + 1) along the row
        prev = np.minimum.accumulate(cur - ar) + ar
    return prev


def restated(q, t, k):
    """(h or -1, [(start, end), ...]) of the issue's semantics: h = min over columns j >= 1 of D[P][j] on the zero-top-row matrix, the ends
    every 0-based column j - 1 with D[P][j] == h in ascending order, each with the smallest s with ed(q, t[s..end]) == h from the
    reversed matrix with top row j."""
    P, n = len(q), len(t)
    if P == 0 or n == 0 or n - P < -k:
        return -1, []
    last = _last_row(q, t, True)[1:]
    h = int(last.min())
    if h > k:
        return -1, []
    locs = []
    for e in np.nonzero(last == h)[0].tolist():
        rev = _last_row(q[::-1], t[max(0, e + 1 - P - h):e + 1][::-1], False)          # (a window longer than P + h costs more than h)
        j = int(np.nonzero(rev == h)[0].max())
        assert j >= 1
        locs.append((e - (j - 1), e))
    return h, locs


@functools.lru_cache(maxsize=None)
def restated_cached(q, t, k):
    h, locs = restated(q, t, k)
    return h, tuple(locs)


def rows(delta, h):
    return max(delta, 0) + 2 * h + 1


words = E.words
body, plant = E.body, E.plant


def _rng(*key):
    return random.Random("hw_locations_cases/" + "/".join(str(x) for x in key))


def spaced(copies, gaps, tail=0):
    """T-gap, copy, T-gap, copy ...: (target, [0-based end of every copy])"""
    out, ends = [], []
    n = 0
    for g, c in zip(gaps, copies):
        out.append("T" * g + c)
        n += g + len(c)
        ends.append(n - 1)
    return "".join(out) + "T" * tail, ends


# ---- a. band classes ---------------------------------------------------------------------------------------------------------------
def group_a():
    """ENDS bands at the class edges (tests/hw_edge_cases.py group a: distance == k, so the ENDS band is the LOCATE band), START bands
    at theirs (its group b), and both again under a threshold far above the distance: LOCATE then runs a wider class than ENDS / START."""
    for c in E.cases("a"):
        R = int(c.name.split("rows")[1].split("_")[0])
        if R not in ENDS_EDGES:
            continue
        lanes = [dict(dist=l["dist"], first=(l["start"], l["end"]), ends_w=words(R)) if "start" in l else dict(dist=l["dist"]) for l in c.lanes]
        yield LCase("a_" + c.name, "a", c.query, list(c.targets), list(c.ks), "ENDS band of %d diagonals" % R, lanes)
    for c in E.cases("b"):
        h = int(c.name[3:])
        if h not in START_EDGES:
            continue
        lanes = [dict(dist=h, first=(l["start"], l["end"]), starts_w=words(2 * h + 1)) for l in c.lanes]
        yield LCase("a_" + c.name, "a", c.query, list(c.targets), list(c.ks), "START band of 2 x %d + 1 diagonals" % h, lanes)
        if 2 * h + 1 <= 128:
            # the same pairs with k so large that LOCATE needs the next class or the one after
            kk = [min((511 - max(len(t) - len(c.query), 0)) // 2, 4 * h) for t in c.targets]
            lanes = [dict(l, locate_w=words(rows(len(t) - len(c.query), k)), ends_w=words(rows(len(t) - len(c.query), h))) for l, t, k in zip(lanes, c.targets, kk)]
            yield LCase("a_wide_" + c.name, "a", c.query, list(c.targets), kk, "distance %d under thresholds %s: LOCATE in a wider class than ENDS" % (h, kk), lanes)


# ---- b. columns --------------------------------------------------------------------------------------------------------------------
def group_b():
    rng = _rng("b")
    b = body(rng, 20)
    P = len(b)
    # one exact copy ending in column e + 1
    targets = ["T" * (e + 1 - P) + b + "T" * 40 for e in BLOCK_ENDS]
    yield LCase("b_block_ends", "b", b, targets, [2] * len(targets), "one end at 30 .. 33 and 62 .. 65", [dict(dist=0, locs=[(e + 1 - P, e)]) for e in BLOCK_ENDS])
    # first eligible column j = P - h (the copy with h bases deleted opens the target) and the last column
    for h in (0, 1, 3):
        d = plant(b, h, "del")
        targets = [d + "T" * 50, "T" * 50 + d, d]
        lanes = [dict(dist=h, ends=[P - h - 1]), dict(dist=h, ends=[50 + P - h - 1]), dict(dist=h, locs=[(0, P - h - 1)])]
        yield LCase("b_first_last_h%d" % h, "b", b, targets, [h + 2, h + 2, h], "end in column P - h, in the last column, and both at once", lanes)
    # two ends in one 32-column block
    s = body(rng, 10)
    t, ends = spaced([s, s], [30, 5], 40)
    yield LCase("b_two_in_block", "b", s, [t], [1], "two ends in columns 33 .. 64", [dict(dist=0, locs=[(e - 9, e) for e in ends])])
    assert ends == [39, 54]
    # far-apart copies with a stretch above h between them: the abandon rule must not fire before the later copy
    b30 = body(rng, 30)
    for h, k in ((0, 0), (0, 6), (2, 2), (2, 9)):
        c = plant(b30, h, "sub")
        for gap in (70, 150, 200):
            t, ends = spaced([c, c, c], [11, gap, gap], 3)
            yield LCase("b_far_h%d_k%d_gap%d" % (h, k, gap), "b", b30, [t], [k], "three copies %d columns apart, every cell between above h" % gap,
                        [dict(dist=h, locs=[(e - 29, e) for e in ends], gap_above=True)])
    # a run of adjacent tied ends: the copy loses its last r bases to T -- the query's tail goes as i insertions and r - i substitutions
    for r in (1, 2, 5):
        t = "T" * 17 + b[:P - r] + "T" * 30
        e0 = 17 + P - r - 1
        yield LCase("b_run%d" % r, "b", b, [t], [r + 1], "%d adjacent ends" % (r + 1), [dict(dist=r, locs=[(17, e0 + i) for i in range(r + 1)])])


# ---- c. degenerate ------------------------------------------------------------------------------------------------------------------
def group_c():
    rng = _rng("c")
    b = body(rng, 24)
    P = len(b)
    for r in COPIES:
        t, ends = spaced([b] * r, [7] * r, 9)
        yield LCase("c_exact_x%d" % r, "c", b, [t], [0], "distance 0, %d copies" % r, [dict(dist=0, locs=[(e - P + 1, e) for e in ends])])
    s2 = plant(b, 2, "sub")
    t, ends = spaced([s2, s2], [5, 40], 5)
    yield LCase("c_h_eq_k", "c", b, [t, t], [2, 1], "distance k, and k + 1: a miss without locations", [dict(dist=2, n_ends=2), dict(dist=2)])
    for P1, n in ((5, 9), (40, 41), (100, 130)):
        yield LCase("c_all_P%d" % P1, "c", "A" * P1, ["C" * n], [P1], "distance P: every column is an end",
                    [dict(dist=P1, locs=[(max(0, e + 1 - P1), e) for e in range(n)])])
    yield LCase("c_P1", "c", "A", ["TTATTAAT", "TTT", "A"], [1, 1, 0], "a query of one base",
                [dict(dist=0, locs=[(2, 2), (5, 5), (6, 6)]), dict(dist=1, locs=[(0, 0), (1, 1), (2, 2)]), dict(dist=0, locs=[(0, 0)])])
    yield LCase("c_n1", "c", "ACG", ["A", "C", "T"], [3, 2, 3], "a target of one base", [dict(dist=2, locs=[(0, 0)]), dict(dist=2, locs=[(0, 0)]), dict(dist=3, locs=[(0, 0)])])
    for k in (1, 4):
        yield LCase("c_short_by_k%d" % k, "c", b, [plant(b, k, "del"), plant(b, k, "del")[:-1]], [k, k], "len(t) - len(q) == -k, and one base less: no kernel",
                    [dict(dist=k, locs=[(0, P - k - 1)]), dict(dist=k + 1)])


# ---- d. tiles ----------------------------------------------------------------------------------------------------------------------
def group_d():
    """many targets on one query; lanes of 1 and 40 ends in one ENDS tile; (pair, end) entries of one pair over two START tiles"""
    for n in TILE_SIZES:
        rng = _rng("d", n)
        b = body(rng, 26)
        targets, lanes = [], []
        for i in range(n):
            h = i % 3
            r = 1 + i % 2
            c = plant(b, h, "sub" if i % 4 < 2 else "del")
            t, ends = spaced([c] * r, [(i * 7) % 5] + [3] * (r - 1), 0)
            targets.append(t + "T" * (62 - len(t)))          # one length: one class, full tiles
            lanes.append(dict(dist=h, ends=ends, ends_w=1))
        yield LCase("d_targets%d" % n, "d", b, targets, [3] * n, "%d targets on one query, 1 or 2 ends each" % n, lanes)
    rng = _rng("d", "ends")
    s = body(rng, 8)
    many, ends40 = spaced([s] * 40, [2] * 40, 0)
    some, ends30 = spaced([s] * 30, [2] * 30, 100)
    one, ends1 = spaced([s], [350], 42)
    assert len(many) == len(some) == len(one) == 400
    yield LCase("d_1_and_40", "d", s, [many, one, some], [0, 0, 0], "lanes of 40, 1 and 30 ends in one tile; 71 (pair, end) entries: some pair's span two START tiles",
                [dict(dist=0, locs=[(e - 7, e) for e in ee], ends_w=8) for ee in (ends40, ends1, ends30)])


def group_e():
    """one query whose two pairs fit 512 diagonals each but not together: the ENDS and LOCATE tiles are cut on the host"""
    rng = _rng("e")
    b = body(rng, 620)
    near = plant(b, 200, "sub")
    far = "T" * 395 + plant(b, 5, "sub") + "T" * 5
    yield LCase("e_host_cut", "e", b, [near, far], [200, 50], "bands of 401 and 501 diagonals, 801 in common",
                [dict(dist=200, first=(0, 619), ends_w=8), dict(dist=5, locs=[(395, 395 + 619)], ends_w=8)])


@functools.lru_cache(maxsize=None)
def cases(group):
    return tuple({"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e}[group]())


ALL_GROUPS = tuple("abcde")


def flatten(case_list):
    """(seqs, q, t, k, owner) for one store, as tests/hw_edge_cases.py flatten"""
    return E.flatten(case_list)[:5]


@functools.lru_cache(maxsize=None)
def expected(group):
    """{(case name, lane): (h, locations)} by the restatement, computed once per process (do not change it)"""
    return {(c.name, i): restated_cached(c.query, t, k) for c in cases(group) for i, (t, k) in enumerate(zip(c.targets, c.ks))}


def ends_tiles(case, group):
    """The ENDS tiles of one query's hits, cut as the host cuts LOCATE tiles (tests/hw_edge_cases.py host_tiles) with the distance in the
    threshold's place: a list of (W, [lanes])."""
    exp = expected(group)
    hits = [i for i in range(len(case.targets)) if exp[case.name, i][0] >= 0]
    P = len(case.query)
    tiles = []
    for W in (1, 2, 4, 8):
        cur, dmax, hmax = None, 0, 0
        for i in hits:
            delta, h = len(case.targets[i]) - P, exp[case.name, i][0]
            if words(rows(delta, h)) != W:
                continue
            d2, h2 = max(dmax, delta), max(hmax, h)
            if cur is not None and len(cur) < 64 and rows(d2, h2) <= 64 * W:
                cur.append(i)
                dmax, hmax = d2, h2
            else:
                cur = [i]
                tiles.append((W, cur))
                dmax, hmax = delta, h
    return tiles


# ---- the random list of the consistency test -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_list(n_pairs=300, seed=20):
    """(seqs, q, t, k): queries of 20 .. 200 bases over ACGT, targets of P - k .. P + 150 bases made of mutated repeats of the query and
    random filler"""
    rng = random.Random("hw_locations_cases/random/%d" % seed)
    seqs, q, t, k = [], [], [], []
    while len(q) < n_pairs:
        P = rng.randint(20, 60) if rng.random() < 0.5 else rng.randint(20, 200)          # (short queries: several copies fit P + 150)
        query = E.rnd(rng, P)
        qi = len(seqs)
        seqs.append(query)
        for _ in range(rng.randint(1, 6)):
            kk = rng.choice((0, 1, 2, 5, 10, 25))
            n = rng.randint(max(1, P - kk), P + 150)
            parts, size, same = [], 0, None
            while size < n:
                if same is not None and rng.random() < 0.6:
                    piece = same          # the copy before again: the same distance, another end
                elif rng.random() < 0.7:
                    c = list(query)
                    for _ in range(rng.choice((0, 0, 1, 2, 4, 8, 30))):
                        i = rng.randrange(len(c))
                        c[i] = rng.choice(("", rng.choice("ACGT"), c[i] + rng.choice("ACGT")))
                    piece = same = "".join(c)
                else:
                    piece = E.rnd(rng, rng.randint(1, 40))
                parts.append(piece)
                size += len(piece)
            q.append(qi)
            t.append(len(seqs))
            seqs.append("".join(parts)[:n])
            k.append(kk)
    return tuple(seqs), tuple(q[:n_pairs]), tuple(t[:n_pairs]), tuple(k[:n_pairs])
