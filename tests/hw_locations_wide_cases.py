"""Designed inputs for isocon_hw_locations_wide (csrc/hw_rows.hpp, hw_loc_wide_host.inc: every best location of an infix pair whose band
exceeds 512 diagonals).  The specification is hw_locations_cases.restated, imported and not restated again; tests/test_hw_locations_wide_core.py
asserts on the CPU that every case is what it claims (band, distance, number of ends, route) and runs the cases through the emulators of the
two kernels; tests/test_gpu_hw_locations_wide.py compares the device with the restatement on every pair.  Fixed seeds, standard library and
numpy only, no library load.

Construction as in tests/hw_edge_cases.py: query bodies over A, C, G, everything else T, so a planted copy with d edits has distance exactly
d and several copies in one target make several ends.

A case = WCase(name, group, query, target, k, route, dist, n_ends): one pair.  route: the kernel its ends come from under the default
switch -- "w1", "w2", "w4" (one lane per pair, 1, 2, 4 query words), "wave" (one wavefront per pair), "narrow" (the band fits: through
isocon_hw_locations) or "none" (no kernel: a miss by the lengths).  dist: the unbounded distance (None: not claimed); n_ends: the ends
the call must report (0 for a miss; None: not claimed)."""
import functools
import random
from collections import namedtuple

import hw_edge_cases as E
import hw_locations_cases as L

WCase = namedtuple("WCase", "name group query target k route dist n_ends")

restated = L.restated
body, plant, spaced = L.body, L.plant, L.spaced

SHORT_QUERIES = (1, 31, 63, 64, 65, 127, 128, 129, 255, 256)
SHORT_TARGETS = (639, 640, 641, 703, 704, 705, 1400)
LONG_QUERIES = (257, 300, 4096, 4100)
TEXT_LOAD_ENDS = (543, 544, 545, 575, 576, 577)          # 31, 32, 33, 63, 64, 65 modulo 64
LIST_SIZES = (1, 63, 64, 65, 130)
ROWS_MAX = 256                                           # kHwlRowsMax of csrc/hw_loc_wide_host.inc


def band(len_q, len_t, k):
    return max(len_t - len_q, 0) + 2 * k + 1


def route_of(len_q, len_t, k, rows_max=ROWS_MAX):
    """hwf_is_narrow of csrc/hw_full_host.inc, then the classes of HwlWide::count"""
    if len_q == 0 or len_t == 0 or len_t - len_q < -k:
        return "none"
    if band(len_q, len_t, k) <= 512:
        return "narrow"
    if len_q > rows_max:
        return "wave"
    return "w1" if len_q <= 64 else "w2" if len_q <= 128 else "w4"


def _rng(*key):
    return random.Random("hw_locations_wide_cases/" + "/".join(str(x) for x in key))


def _case(name, group, query, target, k, dist, n_ends):
    return WCase(name, group, query, target, k, route_of(len(query), len(target), k), dist, n_ends)


def wide_k(len_q, len_t, k):
    """k, or the smallest threshold above it that makes the pair's band exceed 512 diagonals"""
    return max(k, (512 - max(len_t - len_q, 0)) // 2 + 1)


# ---- word and route edges -------------------------------------------------------------------------------------------------------------
def group_edges():
    for P in SHORT_QUERIES:
        rng = _rng("edges", P)
        b = body(rng, P)
        for n in SHORT_TARGETS:
            at = (n - P) // 3
            d = 0 if P < 31 else 1
            t = "T" * at + plant(b, d, "sub") + "T" * (n - P - at)
            assert len(t) == n
            yield _case("edges_q%d_t%d" % (P, n), "edges", b, t, wide_k(P, n, 2), d, 1)
    for P in LONG_QUERIES:
        rng = _rng("edges", P)
        b = body(rng, P)
        t = "T" * 90 + plant(b, 3, "del") + "T" * 113
        assert len(t) == P + 200
        yield _case("edges_q%d" % P, "edges", b, t, P, 3, 1)


# ---- where copies sit ----------------------------------------------------------------------------------------------------------------
def group_copies():
    rng = _rng("copies")
    b = body(rng, 30)
    P = len(b)
    for r in L.COPIES:
        for d, kind in ((0, "sub"), (1, "sub"), (1, "del"), (1, "ins"), (3, "sub"), (3, "del"), (3, "ins")):
            c = plant(b, d, kind)
            t, ends = spaced([c] * r, [57] * r, 700 - r * (57 + len(c)))
            yield _case("copies_x%d_%s%d" % (r, kind, d), "copies", b, t, 3, d, r)
    yield _case("copies_first_column", "copies", b, b + "T" * 611, 2, 0, 1)
    yield _case("copies_last_column", "copies", b, "T" * 611 + b, 2, 0, 1)
    for e in TEXT_LOAD_ENDS:
        yield _case("copies_end%d" % e, "copies", b, "T" * (e + 1 - P) + b + "T" * 70, 2, 0, 1)
    u = body(rng, 15)
    yield _case("copies_overlap", "copies", u + u, "T" * 300 + u * 3 + "T" * 300, 1, 0, 2)
    worse = plant(b, 2, "sub")
    t, _ = spaced([worse, b], [200, 150], 250)
    yield _case("copies_better_after_worse", "copies", b, t, 3, 0, 1)
    t, _ = spaced([b, worse, b], [100, 150, 150], 200)
    yield _case("copies_equal_around_worse", "copies", b, t, 3, 0, 2)
    t, _ = spaced([worse, worse, b, worse], [70, 90, 110, 130], 200)
    yield _case("copies_two_worse_then_better", "copies", b, t, 3, 0, 1)


# ---- every column an end -------------------------------------------------------------------------------------------------------------
def group_all():
    rng = _rng("all")
    yield _case("all_q20_t700", "all", body(rng, 20), "T" * 700, 20, 20, 700)
    yield _case("all_q300_t310", "all", body(rng, 300), "T" * 310, 300, 300, 310)


# ---- misses and thresholds -----------------------------------------------------------------------------------------------------------
def group_thresholds():
    rng = _rng("thresholds")
    b = body(rng, 40)
    t = "T" * 400 + plant(b, 3, "sub") + "T" * 300
    yield _case("thr_k_below", "thresholds", b, t, 2, 3, 0)
    yield _case("thr_k_equal", "thresholds", b, t, 3, 3, 1)
    long = body(rng, 600)
    yield _case("thr_short_by_k", "thresholds", long, long[:300], 300, 300, None)
    yield _case("thr_short_by_k_plus_1", "thresholds", long, long[:299], 300, None, 0)
    yield _case("thr_empty_query", "thresholds", "", t, 5, None, 0)
    yield _case("thr_empty_target", "thresholds", b, "", 50, None, 0)


# ---- lanes of one wave that finish apart ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lane_list(n_pairs):
    """(query, [target], [k], [ends the pair must report]): wide pairs of one 30-base query, targets of 600 to 1 500 bases in mixed order"""
    rng = _rng("lanes", n_pairs)
    b = body(rng, 30)
    targets, ks, n_ends = [], [], []
    for i in range(n_pairs):
        n = rng.randint(600, 1500)
        kind = i % 4
        if kind == 3:          # a miss: no copy within k
            t = "T" * n if i % 8 == 3 else "T" * 50 + plant(b, 3, "sub") + "T" * (n - 80)
            targets.append(t); ks.append(2); n_ends.append(0)
            continue
        r = 1 + (i * 7) % 5
        c = plant(b, kind, "sub")
        gaps = [rng.randint(40, (n - r * 30) // r) for _ in range(r)]
        t, _ = spaced([c] * r, gaps, 0)
        targets.append(t + "T" * (n - len(t))); ks.append(3); n_ends.append(r)
    return b, tuple(targets), tuple(ks), tuple(n_ends)


def group_lanes():
    for size in LIST_SIZES:
        b, targets, ks, n_ends = lane_list(size)
        for i, (t, k, e) in enumerate(zip(targets, ks, n_ends)):
            yield _case("lanes%d_%d" % (size, i), "lanes", b, t, k, None, e)


# ---- narrow and wide pairs interleaved -----------------------------------------------------------------------------------------------
def group_mixed():
    rng = _rng("mixed")
    b = body(rng, 30)
    near = "T" * 20 + b + "T" * 30 + b + "T" * 10          # 120 bases: narrow under a small k
    far = "T" * 500 + b + "T" * 200 + plant(b, 1, "sub") + "T" * 100
    b200 = body(rng, 200)
    t200 = "T" * 30 + plant(b200, 4, "sub") + "T" * 70          # 300 bases: narrow under k = 10, wide under k = 250
    yield _case("mixed_narrow_a", "mixed", b, near, 3, 0, 2)
    yield _case("mixed_wide_a", "mixed", b, far, 3, 0, 1)
    yield _case("mixed_same_pair_k10", "mixed", b200, t200, 10, 4, 1)
    yield _case("mixed_wide_b", "mixed", b, far, 0, 0, 1)
    yield _case("mixed_same_pair_k250", "mixed", b200, t200, 250, 4, 1)
    yield _case("mixed_narrow_miss", "mixed", b, near[:25], 2, None, 0)
    yield _case("mixed_wide_c", "mixed", b200, "T" * 400 + b200 + "T" * 100 + b200, 5, 0, 2)
    yield _case("mixed_narrow_b", "mixed", b, near, 0, 0, 2)


GROUPS = {"edges": group_edges, "copies": group_copies, "all": group_all, "thresholds": group_thresholds, "lanes": group_lanes, "mixed": group_mixed}
ALL_GROUPS = tuple(GROUPS)


@functools.lru_cache(maxsize=None)
def cases(group):
    return tuple(GROUPS[group]())


@functools.lru_cache(maxsize=None)
def expected(group):
    """[(h, locations)] of the group's cases by the restatement, computed once per process (do not change it)"""
    return tuple(L.restated_cached(c.query, c.target, c.k) for c in cases(group))


def flatten(case_list):
    """(seqs, q, t, k) for one store: equal strings share an entry"""
    seqs, index, q, t, k = [], {}, [], [], []
    for c in case_list:
        for s, out in ((c.query, q), (c.target, t)):
            if s not in index:
                index[s] = len(seqs)
                seqs.append(s)
            out.append(index[s])
        k.append(c.k)
    return seqs, q, t, k


# ---- the random list -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_list(n_pairs=300, seed=7):
    """(seqs, q, t, k): queries of 1 to 400 bases over ACGT, targets of 520 to 1 600, k from 0 to len(q); half the targets carry 1 to 4
    mutated copies of the query"""
    rng = random.Random("hw_locations_wide_cases/random/%d" % seed)
    seqs, q, t, k = [], [], [], []
    for _ in range(n_pairs):
        P = rng.randint(1, 400) if rng.random() < 0.7 else rng.randint(1, 70)
        query = E.rnd(rng, P)
        n = rng.randint(520, 1600)
        target = list(E.rnd(rng, n))
        if rng.random() < 0.5:
            same = None
            for _ in range(rng.randint(1, 4)):
                if same is None or rng.random() < 0.5:
                    c = list(query)
                    for _ in range(rng.choice((0, 0, 1, 2, 5, 20))):
                        i = rng.randrange(len(c))
                        c[i] = rng.choice(("", rng.choice("ACGT"), c[i] + rng.choice("ACGT")))
                    same = "".join(c)
                at = rng.randrange(0, max(1, n - len(same)))
                target[at:at + len(same)] = same
        target = "".join(target)[:n]
        q.append(len(seqs)); seqs.append(query)
        t.append(len(seqs)); seqs.append(target)
        k.append(rng.choice((0, 1, 3, P // 4, P // 2, P)) if rng.random() < 0.7 else rng.randint(0, P))
    return tuple(seqs), tuple(q), tuple(t), tuple(k)
