"""numpy restatement of what the bound kernel leaves beside the matrix (isocon_amd/csrc/qgram_mm.hpp: hub scores, row / column minima)
and of the seed pairs proposed from it (k_qgram_seed_pairs), written from the rules and not from the kernels (test infrastructure;
tests/test_gpu_qgram_seed_tables.py compares isocon_qgram_seed_tables with it word by word).

Rules.  Roles: one set -- every entry a target, the queries the entries that are not converged; two sets -- the targets is_target, the
queries the rest.  Slot s of the shard is the entry q = shard_entries(...)[s], its window the columns p = q + 1 .. q + rlen[s] (lengths
within 63, at most `depth` of them), the byte of a window pair min(255, B[q, p]).
  score[x]      window pairs with x at either end whose byte is <= hub_bound (roles play no part)
  rowmin[s][c]  over the window's columns p with (p // tile) % seeds == c, q a query, p a target: the smallest (byte, p) as
                byte << 32 | (p - q - 1); all ones: none
  colmin[p][c]  over the slots s whose window holds p with (s // tile) % seeds == c, p a query, q(s) a target: the smallest
                (byte, q(s)) as byte << 32 | q(s); all ones: none
  pairs of x    (x, x + 1 + e) for every rowmin entry of x's slot that is not all ones, in class order; then for g < col_classes the
                smallest of colmin[x][g], colmin[x][g + col_classes], ...: (q, x) with q its low word unless row q's candidate for the class
                (x // tile) % seeds is x itself.  known[x]: the other ends in that order, then 0xffffffff."""
import numpy as np

ONES = 2 ** 64 - 1
NONE32 = 0xffffffff


def shard_entries(q_begin, q_end, q_stride=1, q_block=1):
    """the entries a shard owns, in slot order: q_begin <= x < q_end with (x - q_begin) mod q_stride < q_block"""
    return [x for x in range(q_begin, q_end) if (x - q_begin) % q_stride < q_block]


def roles(n, is_converged=None, is_target=None):
    """(is_query, is_target) as boolean arrays"""
    if is_target is not None:
        t = np.asarray(is_target).astype(bool)
        return ~t, t
    q = np.ones(n, bool) if is_converged is None else ~np.asarray(is_converged).astype(bool)
    return q, np.ones(n, bool)


def window_lengths(lens, qs, depth):
    """rlen[s]: the entries behind q(s) whose length is within 63 of its own, at most `depth`"""
    lens = np.asarray(lens)
    out = []
    for q in qs:
        hi = int(np.searchsorted(lens, lens[q] + 63, "right"))
        out.append(min(max(hi - q - 1, 0), depth))
    return out


def col_classes_of(seeds, q_stride, q_block, override=None):
    if override in (1, 2, seeds):
        return override
    ranks = max(1, q_stride // q_block)
    cc = seeds
    while cc > 1 and cc * ranks > seeds:
        cc //= 2
    return cc


def seed_tables(lens, B, is_converged, is_target, shard, depth, seeds, hub_bound, tile, col_classes):
    """shard = (q_begin, q_end, q_stride, q_block).  Returns a dict: qs, rlen, score int64[n], rowmin / colmin as lists of lists of
    Python ints, pairs (list of (a, b) in the order of the entries), known (per entry the list of other ends), and the number of window
    bytes <= hub_bound."""
    n = len(lens)
    q_begin, q_end, q_stride, q_block = shard
    qs = shard_entries(q_begin, min(q_end, n), q_stride, q_block)
    rlen = window_lengths(lens, qs, depth)
    isq, ist = roles(n, is_converged, is_target)
    score = np.zeros(n, np.int64)
    rowmin = [[ONES] * seeds for _ in qs]
    col_byte = np.full((n, seeds), 256, np.int64)          # (byte, q) of colmin: 256 = none yet
    col_q = np.zeros((n, seeds), np.int64)
    hub_pairs = 0
    for s, q in enumerate(qs):
        if rlen[s] == 0:
            continue
        p = np.arange(q + 1, q + 1 + rlen[s])
        b = np.minimum(B[q, p], 255).astype(np.int64)
        hub = b <= hub_bound
        score[q] += int(hub.sum())
        score[p] += hub
        hub_pairs += int(hub.sum())
        if isq[q]:
            for c in range(seeds):
                ok = ((p // tile) % seeds == c) & ist[p]
                if ok.any():
                    m = int(b[ok].min())
                    first = int(p[ok & (b == m)][0])          # the lower column wins
                    rowmin[s][c] = (m << 32) | (first - q - 1)
        if ist[q]:
            c = (s // tile) % seeds
            better = isq[p] & (b < col_byte[p, c])          # rows come in ascending q: an equal byte of a later row does not replace
            col_byte[p[better], c] = b[better]
            col_q[p[better], c] = q
    colmin = [[ONES if col_byte[x, c] == 256 else (int(col_byte[x, c]) << 32) | int(col_q[x, c]) for c in range(seeds)] for x in range(n)]
    slot_of = {q: s for s, q in enumerate(qs)}
    pairs, known = [], []
    for x in range(n):
        mine = []
        if x in slot_of:
            for c in range(seeds):
                v = rowmin[slot_of[x]][c]
                if v != ONES:
                    mine.append((x, x + 1 + (v & NONE32)))
        for g in range(col_classes):
            v = min(colmin[x][c] for c in range(g, seeds, col_classes))
            if v == ONES:
                continue
            q = v & NONE32
            r = rowmin[slot_of[q]][(x // tile) % seeds]
            if r != ONES and q + 1 + (r & NONE32) == x:
                continue          # row q proposes this very pair
            mine.append((q, x))
        pairs += mine
        known.append([b if a == x else a for a, b in mine])
    return {"qs": qs, "rlen": rlen, "score": score, "rowmin": rowmin, "colmin": colmin, "pairs": pairs, "known": known, "hub_pairs": hub_pairs}
