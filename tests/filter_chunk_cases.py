"""Designed chunks for the two block-filter kernels of the nearest-neighbour main pass (isocon_amd/csrc/nn_filter.hpp: k_nn_block_filter,
k_nn_block_filter2) and a restatement of what they must do with them (tests/test_gpu_filter_chunks.py compares the device with it through
isocon_block_filter_chunks, tests/test_filter_chunk_cases.py asserts on the CPU that every case sits where it claims).  Fixed seeds, numpy
and tests/qgram_ref.block_count only, nothing of the library's.

The rule.  A list word is partner | bit 30 (the owner's threshold applies) | bit 31 (the partner's applies); the pair's threshold k is -1,
raised to each threshold that applies, clamped to kcap.  A pair survives the first pass iff block_count(owner, partner, s=4) <= k.  With np
survivors of a chunk of `count` pairs: np >= list_min and (no second pass or 2 np >= count) -> they stay a chunk of the chunk's class for
the table kernels; else second pass and np >= 16 -> ceil(np / 64) tasks of the second pass, whose survivors (block_count(.., s=2) <= k as
well) join the flat pairs; else the np pairs join the flat pairs as they are."""
import functools
import operator
from collections import namedtuple

import numpy as np

from tests import qgram_ref

# constants of the kernels, restated (csrc/nn_filter.hpp, csrc/nn_list.hpp): the tests assert the cases against these
NNF_GRID = 2048               # workgroups of the first pass: more chunks than this and a workgroup takes a second one
NNF_GRID2 = 1024              # workgroups of the second pass, four waves (tasks) each
PASS2_MIN = 16
LIST_MIN = 256                # the product's list_min (NN_LIST_MIN)
CHUNK_MAX = 2048 + 63         # the most pairs the list builder hands over as one chunk (NN_LIST_CHUNK + 63: it asks after every 64 positions)
PIECE = 16                    # text dwords per piece of the count loop

OWNER_BIT, PARTNER_BIT = 1 << 30, 1 << 31
INDEX_MASK = (1 << 30) - 1

# one call of the entry: the store's sequences, thr[n], the chunks [(owner, narrow, uint32 list words)], kcap, list_min
Call = namedtuple("Call", "name seqs thr chunks kcap list_min")
# what a chunk does: its route ("table", "second", "flat"), the survivors of the first pass and of the chunk (boolean masks over its words)
ChunkResult = namedtuple("ChunkResult", "route np keep1 final")

BASES = "ACGT"


def dwords(length, s):
    """text dwords all of whose probes (stride s) lie inside a sequence: what one lane of the count loop walks"""
    return (length - (24 - s)) // 16 + 1 if length >= 24 - s else 0


def pieces(length, s):
    return (dwords(length, s) + PIECE - 1) // PIECE


@functools.lru_cache(maxsize=None)
def count(owner, partner, s):
    return qgram_ref.block_count(owner, partner, s=s)


def pair_threshold(word, thr, owner, kcap):
    k = -1
    if word & OWNER_BIT:
        k = max(k, int(thr[owner]))
    if word & PARTNER_BIT:
        k = max(k, int(thr[word & INDEX_MASK]))
    return min(k, kcap)


def route_of(np_, cnt, list_min, second, ge=operator.ge, pass2_min=PASS2_MIN):
    if np_ >= list_min and (not second or ge(2 * np_, cnt)):
        return "table"
    if second and np_ >= pass2_min:
        return "second"
    return "flat"


def expect(call, second, count=count, le=operator.le, pair_threshold=pair_threshold, ge=operator.ge, pass2_min=PASS2_MIN):
    """-> dict: `per_chunk` [ChunkResult], `chunks` sorted [(narrow, owner, sorted list words)] left for the tables, `flat` sorted
    [(owner, partner)], and the counters of the entry.  The keyword arguments are the pieces of the rule (the tests swap one at a time
    to show that the cases notice)."""
    per_chunk, chunks, flat = [], [], []
    c = dict(f_chunks=0, f_chunks_narrow=0, n_small=0, f_rejected=0, f_rejected2=0, f_listed=0, f_narrow_listed=0, f_tasks=0, overflow=0)
    for owner, narrow, words in call.chunks:
        x = call.seqs[owner]
        ks = [pair_threshold(int(w), call.thr, owner, call.kcap) for w in words]
        ys = [call.seqs[int(w) & INDEX_MASK] for w in words]
        keep1 = np.array([le(count(x, y, 4), k) for y, k in zip(ys, ks)], dtype=bool)
        n1 = int(keep1.sum())
        route = route_of(n1, len(words), call.list_min, second, ge, pass2_min)
        final = keep1.copy()
        c["f_rejected"] += len(words) - n1
        if route == "table":
            chunks.append((int(narrow), int(owner), sorted(int(w) for w in words[keep1])))
            c["f_chunks_narrow" if narrow else "f_chunks"] += 1
            c["f_listed"] += n1
            c["f_narrow_listed"] += n1 if narrow else 0
        else:
            if route == "second":
                c["f_tasks"] += (n1 + 63) // 64
                for i in np.flatnonzero(keep1):
                    final[i] = le(count(x, ys[i], 2), ks[i])
                c["f_rejected2"] += n1 - int(final.sum())
            c["n_small"] += int(final.sum())
            flat += [(int(owner), int(w) & INDEX_MASK) for w in words[final]]
        per_chunk.append(ChunkResult(route, n1, keep1, final))
    return dict(c, per_chunk=per_chunk, chunks=sorted(chunks), flat=sorted(flat))


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------

def random_seq(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def substitute(s, positions):
    """s with another base (the next of ACGT) at every position"""
    t = list(s)
    for p in positions:
        t[p] = BASES[(BASES.index(t[p]) + 1) % 4]
    return "".join(t)


def spaced(s, d, first=4, step=8):
    """d substitutions `step` apart: each spoils one counted gram of either grid"""
    return substitute(s, [first + step * i for i in range(d)])


def scattered(rng, s, d, hi=None):
    return substitute(s, sorted(rng.choice(hi or len(s), d, replace=False).tolist()))


def _words(partners, bits):
    return (np.asarray(partners, dtype=np.int64) | np.asarray(bits, dtype=np.int64)).astype(np.uint32)


class _Store(object):
    """the sequences of a call with their thresholds, in the order they were added"""

    def __init__(self):
        self.seqs, self.thr = [], []

    def add(self, s, thr=0):
        self.seqs.append(s)
        self.thr.append(thr)
        return len(self.seqs) - 1

    def call(self, name, chunks, kcap=64, list_min=LIST_MIN):
        return Call(name, list(self.seqs), np.asarray(self.thr, dtype=np.int32), [(o, n, np.asarray(w, dtype=np.uint32)) for o, n, w in chunks], kcap, list_min)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

LENGTHS = (1, 7, 8, 19, 20, 21, 35, 36, 37, 255, 256, 257, 260, 275, 276, 277, 291, 292) + tuple(range(500, 531))
LENGTHS_2 = (22, 38, 278, 294)          # the first lengths with 1, 2, 17 and 18 dwords on the 2-base grid (the list above has those of the 4-base grid)


def case_lengths():
    """Owners of about 300 bases (and degenerate ones) over chunks whose waves of 64 mix partner lengths on both sides of every step of the
    dword counts of both grids and of a 16-dword piece; the first wave of every chunk is 63 partners of at most 37 bases and one of 530."""
    rng = np.random.default_rng(101)
    S = _Store()
    master = random_seq(rng, 530)
    partners = []
    for L in LENGTHS + LENGTHS_2:
        for v in range(3):
            p = master[:L]
            if v and L >= 8:
                p = scattered(rng, p, min(L // 8, (2, 9)[v - 1]))
            partners.append(S.add(p, thr=int(rng.integers(0, 12))))
    short = [S.add(scattered(rng, master[:L], 1), thr=int(rng.integers(0, 4))) for L in (19, 20, 21, 35, 36, 37) * 11][:63]
    long_one = S.add(scattered(rng, master, 6), thr=6)
    owners = [S.add(master[:300], thr=3), S.add(scattered(rng, master[:300], 5), thr=8)]
    owners += [S.add(master[:L], thr=2) for L in range(0, 9)]          # no gram at all below 8 bases: every probe absent; exactly one gram at 8
    owners += [S.add("A" * 300, thr=5), S.add(S.seqs[partners[-1]], thr=4)]          # a homopolymer; an exact copy of a partner (530 bases)
    chunks = []
    for j, o in enumerate(owners):
        order = rng.permutation(partners).tolist()
        ps = short[:31] + [long_one] + short[31:] + order
        bits = [(OWNER_BIT, PARTNER_BIT, OWNER_BIT | PARTNER_BIT)[(i + j) % 3] for i in range(len(ps))]
        chunks.append((o, j & 1, _words(ps, bits)))
    return [S.call("lengths", chunks, kcap=64, list_min=32)]


def _edge_pool(rng, owner):
    """partners of one owner with their counts on both grids: designed ones (count = number of spaced substitutions) and randomly mutated ones
    (the grids disagree on a third of them)"""
    pool = [spaced(owner, d) for d in (0, 1, 31, 32, 63) for _ in range(1)]
    pool += [spaced(owner, d, first=5 + v, step=8 + (v & 1)) for d in (1, 31, 32, 63) for v in range(1, 6)]
    # one more substitution behind the last gram of the 4-base grid (588 .. 595) and inside the 2-base grid's (590 .. 597): count c - 1 and c
    pool += [substitute(spaced(owner, c - 1), [596]) for c in (1, 31, 32, 63)]
    # ... and the other way round: 596 bases are 37 text dwords on the 4-base grid and 36 on the 2-base grid, which never sees a substitution at 590
    pool += [substitute(spaced(owner, c), [590])[:596] for c in (0, 5, 30, 31)]
    pool += [scattered(rng, owner, int(d)) for d in rng.integers(1, 70, 260)]
    for _ in range(40):          # with insertions and deletions
        t = list(scattered(rng, owner, int(rng.integers(1, 30))))
        for p in sorted(rng.choice(len(t) - 1, int(rng.integers(1, 12)), replace=False).tolist(), reverse=True):
            if p & 1:
                del t[p]
            else:
                t.insert(p, BASES[p % 4])
        pool.append("".join(t)[:600])
    return list(dict.fromkeys(pool))


def case_edge_k():
    """Every pair shape at the last threshold that keeps it and the first that rejects it, on the 4-base grid and -- inside chunks of the
    second pass -- on the 2-base grid, with the threshold coming from the partner (bit 31), the owner (bit 30), both (the larger on either
    side) and from kcap below both."""
    rng = np.random.default_rng(202)
    owner = random_seq(rng, 600)
    pool = _edge_pool(rng, owner)
    counts = [(count(owner, p, 4), count(owner, p, 2)) for p in pool]
    calls = []
    # (a) the threshold is the partner's: bit 31 alone, or both bits under an owner with threshold 0
    S = _Store()
    o = S.add(owner, thr=0)
    words = []
    for p, (c4, c2) in zip(pool, counts):
        for k in sorted({c4, c4 - 1, c2, c2 - 1}):
            if 0 <= k <= 64:
                i = S.add(p, thr=k)
                words.append(i | PARTNER_BIT | (OWNER_BIT if len(words) & 1 else 0))
            elif k == -1:
                words.append(S.add(p, thr=9))          # neither bit: k = -1, rejected even at count 0
    words = np.asarray(words, dtype=np.uint32)
    chunks = [(o, j & 1, words[at:at + 150]) for j, at in enumerate(range(0, len(words), 150))]
    calls.append(S.call("edge_k/partner", chunks))
    # (b) the threshold is the owner's: bit 30 alone, or both bits over partners with a smaller threshold
    S = _Store()
    idx = [S.add(p, thr=0) for p in pool]
    chunks = []
    for T in sorted({k for c4, c2 in counts for k in (c4, c4 - 1, c2, c2 - 1) if 0 <= k <= 64}):
        near = [i for i, (c4, c2) in zip(idx, counts) if T in (c4, c4 - 1, c2, c2 - 1)]
        if len(near) < 2:
            continue
        o = S.add(owner, thr=T)
        bits = [OWNER_BIT | (PARTNER_BIT if j & 1 else 0) for j in range(len(near))]
        # (partners kept on both grids pad the chunk to the second pass's 16 survivors where the threshold decides on few)
        pad = [i for i, (c4, c2) in zip(idx, counts) if max(c4, c2) < T - 1][:24]
        chunks.append((o, len(chunks) & 1, _words(near + pad, bits + [OWNER_BIT] * len(pad))))
    calls.append(S.call("edge_k/owner", chunks))
    # (c) kcap = 31 below both thresholds
    S = _Store()
    o = S.add(owner, thr=40)
    near = [S.add(p, thr=50 if j & 1 else 33) for j, (p, (c4, c2)) in enumerate(zip(pool, counts)) if min(c4, c2) <= 33]
    words = _words(near, [(OWNER_BIT, PARTNER_BIT, OWNER_BIT | PARTNER_BIT)[j % 3] for j in range(len(near))])
    calls.append(S.call("edge_k/kcap", [(o, j & 1, words[at:at + 120]) for j, at in enumerate(range(0, len(words), 120))], kcap=31))
    return calls


def first_piece_count(owner, partner, s):
    """the count after the first 16 text dwords (the greedy count of a prefix is the count of the prefix)"""
    return count(owner, partner[:264 - s], s)


def case_early_exit():
    """Waves that may leave the count loop after the first piece and waves that one lane keeps in it to the end of a 530-base text: whether a
    pair is kept must not depend on when the loop stops."""
    rng = np.random.default_rng(303)
    S = _Store()
    owner = random_seq(rng, 530)
    o = S.add(owner, thr=0)
    far = [S.add(random_seq(rng, 530), thr=int(rng.integers(0, 4))) for _ in range(64 + 63 + 63)]          # rejected inside the first piece
    late_rejected = S.add(substitute(owner, [510]), thr=0)          # its one unfound gram lies in the last dword that counts
    late_kept = S.add(substitute(owner, [510]), thr=1)
    w0 = far[:64]
    w1 = far[64:96] + [late_rejected] + far[96:127]
    w2 = far[127:150] + [late_kept] + far[150:190]
    # the 2-base grid: 63 pairs that only the second pass rejects, inside its first piece, and one lane decided in the last dword -- substitutions
    # at 496 and 499 are one counted gram of the 4-base grid (492; 496 is skipped, 500 is clean) and two of the 2-base grid (490, 498)
    merged = substitute(owner, [496, 499])
    early2 = []
    while len(early2) < 126:
        p = scattered(rng, owner, int(rng.integers(4, 24)), hi=200)
        c4, c2 = count(owner, p, 4), count(owner, p, 2)
        if c2 > c4:
            early2.append(S.add(p, thr=c2 - 1))
    g0 = early2[:40] + [S.add(merged, thr=1)] + early2[40:63]          # rejected by the second pass alone, at the end of the text
    g1 = early2[63:80] + [S.add(merged, thr=2)] + early2[80:126]         # kept, known at the end of the text
    chunks = [(o, 0, _words(w0 + w1 + w2, [PARTNER_BIT] * 192)), (o, 1, _words(g0, [PARTNER_BIT | OWNER_BIT] * 64)), (o, 0, _words(g1, [PARTNER_BIT] * 64))]
    return [S.call("early_exit", chunks)]


SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, CHUNK_MAX)


def case_sizes():
    """Chunks of every size around a wave, a workgroup's round of four waves, a chunk of the builder and its maximum; list_min 256 and 32."""
    rng = np.random.default_rng(404)
    S = _Store()
    base = random_seq(rng, 120)
    partners = [S.add(scattered(rng, base, int(d)), thr=int(t)) for d, t in zip(rng.integers(0, 9, CHUNK_MAX), rng.integers(0, 8, CHUNK_MAX))]
    chunks = []
    for j, n in enumerate(SIZES):
        o = S.add(scattered(rng, base, j % 3), thr=int(rng.integers(1, 6)))
        ps = rng.permutation(partners)[:n].tolist()
        chunks.append((o, j & 1, _words(ps, [(PARTNER_BIT, OWNER_BIT | PARTNER_BIT, OWNER_BIT)[(i * 7 + j) % 3] for i in range(n)])))
    return [S.call("sizes/list_min_256", chunks, list_min=256), S.call("sizes/list_min_32", chunks, list_min=32)]


# (pairs of the chunk, survivors of the first pass) with list_min = 32: np on both sides of list_min, 2 np on both sides of the chunk's count,
# np on both sides of the second pass's 16 and of its tasks of 64, np = 0
ROUTING_SHAPES = ((40, 31), (40, 32), (81, 40), (80, 40), (79, 40), (30, 15), (30, 16), (200, 64), (200, 65), (300, 129), (20, 0), (50, 10), (18, 3), (70, 33), (64, 64))


def case_routing():
    """Chunks whose number of survivors is set by their partners' thresholds: a partner is the owner's text with two substitutions (count 2 on
    both grids), kept under threshold 2 and rejected under threshold 1."""
    rng = np.random.default_rng(505)
    S = _Store()
    base = random_seq(rng, 200)
    variants = [substitute(base, [4 + 8 * a, 4 + 8 * b]) for a in range(23) for b in range(a + 1, 23)]
    variants = [variants[i] for i in rng.permutation(len(variants))]
    keep = [S.add(p, thr=2) for p in variants[:129]]
    rej = [S.add(p, thr=1) for p in variants[:171]]
    chunks = []
    for narrow in (0, 1):
        for rep in range(2):
            for n, kept in ROUTING_SHAPES:
                o = S.add(base, thr=0)
                ps = rng.permutation(keep[:kept] + rej[:n - kept]).tolist()
                chunks.append((o, narrow, _words(ps, [PARTNER_BIT | (OWNER_BIT if rep else 0)] * n)))
    return [S.call("routing", chunks, list_min=32)]


def case_queue():
    """More chunks than the first pass has workgroups and more tasks than the second pass has waves: a workgroup (a wave) takes another chunk
    (task) over the bitmap, the survivor buffer and the counter the last one left.  Consecutive chunks alternate between two families of
    owners with disjoint gram sets."""
    rng = np.random.default_rng(606)
    S = _Store()
    fam = [random_seq(rng, 80), random_seq(rng, 80)]
    owners = [[S.add(scattered(rng, fam[f], 1), thr=0) for _ in range(40)] for f in (0, 1)]
    partners = [[S.add(scattered(rng, fam[f][:int(L)], int(d)), thr=int(t)) for L, d, t in zip(rng.integers(40, 81, 2400), rng.integers(0, 3, 2400), rng.integers(1, 4, 2400))]
                for f in (0, 1)]
    foreign = [[S.add(random_seq(rng, int(L)), thr=1) for L in rng.integers(40, 81, 400)] for f in (0, 1)]
    chunks = []
    cursor = {}
    for c in range(4400):
        f, j = c & 1, (c >> 1) % 40
        n = int(rng.integers(32, 41)) if c < 2200 else int(rng.integers(24, 29))
        at, nth = cursor.get((f, j), (0, 0))          # every (owner, partner) pair once: an owner walks through its family's partners
        cursor[f, j] = (at + n - 1, nth + 1)
        ps = [partners[f][at + i] for i in range(n - 1)] + [foreign[f][nth]]
        chunks.append((owners[f][j], (c >> 2) & 1, _words(ps, [PARTNER_BIT] * n)))
    return [S.call("queue", chunks, list_min=LIST_MIN)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Call, in a fixed order"""
    out = {}
    for make in (case_lengths, case_edge_k, case_early_exit, case_sizes, case_routing, case_queue):
        for call in make():
            out[call.name] = call
    return out


@functools.lru_cache(maxsize=None)
def expected(name, second):
    """expect() of a case, computed once and shared (treat it as read-only)"""
    return expect(cases()[name], second)


# ---- the inputs of the randomised filter stress (scripts/stress_filter.py; tests/test_gpu_filter_chunks.py runs a fixed-seed slice) ------

def stress_lowc(rng):
    n, L = rng.randint(200, 1500), rng.randint(60, 900)
    base = "".join(rng.choice("AC") for _ in range(L))
    seqs = []
    for i in range(n):
        s = list(base)
        for _ in range(rng.randint(0, 20)):
            p = rng.randrange(len(s)); op = rng.random()
            if op < 0.4: s[p] = rng.choice("AC")
            elif op < 0.7: s.insert(p, rng.choice("AC"))
            else: del s[p]
        seqs.append("".join(s) or "A")
    return seqs


def stress_homo(rng):
    n = rng.randint(200, 1200)
    runs = [(rng.choice("ACGT"), rng.randint(1, 14)) for _ in range(rng.randint(20, 120))]
    return ["".join(c * max(1, l + rng.choice([0, 0, 0, 1, -1])) for c, l in runs) for i in range(n)]


def stress_edges(rng):
    n = rng.randint(100, 800)
    L = rng.choice([19, 20, 21, 35, 36, 37, 255, 256, 257, 271, 272, 273])
    base = "".join(rng.choice("ACGT") for _ in range(L))
    seqs = []
    for i in range(n):
        s = list(base)
        for _ in range(rng.randint(0, 4)):
            p = rng.randrange(len(s)); s[p] = rng.choice("ACGT")
        if rng.random() < 0.3: s.insert(rng.randrange(len(s)), rng.choice("ACGT"))
        seqs.append("".join(s))
    return seqs


STRESS_GENERATORS = {"lowc": stress_lowc, "homo": stress_homo, "edges": stress_edges}
