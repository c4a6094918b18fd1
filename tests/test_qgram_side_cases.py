"""The designed set of tests/qgram_side_cases.py sits where it claims, by the restatements alone (tests/qgram_ref.py, tests/qgram_seed_ref.py):
every condition below is a coverage requirement of tests/test_gpu_qgram_seed_tables.py.  No GPU, no library."""
import functools

import numpy as np

import qgram_seed_ref as S
import qgram_side_cases as C

SEEDS, HUB, TILE = 4, 36, 256          # the kernel's constants today (the GPU test takes them from the entry and asserts these)
ONES = S.ONES


def _lens():
    return np.array([len(s) for s in C.sequences()])


@functools.lru_cache(maxsize=None)
def _tables(role, shard_name, depth, classes=None):
    seqs = C.sequences()
    n = len(seqs)
    conv, targ = C.role_settings(n)[role]
    shard = C.shard(shard_name, n)
    cc = S.col_classes_of(SEEDS, shard[2], shard[3], classes)
    return S.seed_tables(_lens(), C.bound_matrix(), conv, targ, shard, depth, SEEDS, HUB, TILE, cc)


def _windows(role, depth):
    """full shard: (q, p[], byte[], eligible as a row[], eligible as a column[]) per row with a window"""
    n = len(C.sequences())
    B = C.bound_matrix()
    isq, ist = S.roles(n, *C.role_settings(n)[role])
    qs = list(range(n))
    for q, rl in zip(qs, S.window_lengths(_lens(), qs, depth)):
        if rl:
            p = np.arange(q + 1, q + 1 + rl)
            yield q, p, np.minimum(B[q, p], 255), isq[q] & ist[p], ist[q] & isq[p]


def _tie_kinds(at):
    """how the positions `at` (ascending) of a minimum are spread: in one 16-chunk, in two chunks of a tile, in two tiles"""
    kinds = set()
    chunks, tiles = at // 16, at // TILE
    if len(set(chunks.tolist())) < len(at):
        kinds.add("chunk")
    for t in set(tiles.tolist()):
        if len(set(chunks[tiles == t].tolist())) > 1:
            kinds.add("tile")
    if len(set(tiles.tolist())) > 1:
        kinds.add("class")
    return kinds


def test_size_and_order():
    seqs = C.sequences()
    n = len(seqs)
    assert n % TILE not in (0, TILE - 1) and n % 16 != 0
    assert (n + TILE - 1) // TILE >= SEEDS + 2
    assert all(len(x) <= len(y) for x, y in zip(seqs, seqs[1:])) and len(set(seqs)) == n
    assert all(300 <= len(s) <= 340 for s in seqs[:C.N_MAIN])
    assert set("".join(seqs)) == set("ACGT")


def test_settings_cover_what_the_gpu_test_must_cross():
    st = C.SETTINGS
    assert len(set(st)) == len(st)
    cyclic = ("cyclic0", "cyclic1", "cut")
    for r in C.ROLE_NAMES:          # every role setting on the full and on a block-cyclic shard
        assert any(x[0] == r and x[1] == "full" for x in st) and any(x[0] == r and x[1] in cyclic for x in st)
    for s in C.SHARDS:              # every shard and every depth with the uniform and a non-uniform role setting
        assert any(x[0] == "uniform" and x[1] == s for x in st) and any(x[0] != "uniform" and x[1] == s for x in st)
    for d in C.DEPTHS:
        assert any(x[0] == "uniform" and x[2] == d for x in st) and any(x[0] != "uniform" and x[2] == d for x in st)
    assert all(x[2] == 2 ** 32 for x in st if x[0].startswith("two_set"))          # depths in the 1-set settings only
    for c in (1, 2):
        assert any(x[3] == c and x[1] == "full" for x in st)
    n = len(C.sequences())
    got = {S.col_classes_of(SEEDS, *C.shard(x[1], n)[2:]) for x in st if x[3] is None}
    assert got == {4, 2, 1}          # the shards make col_classes 4, 2 and 1
    roles = C.role_settings(n)
    conv = roles["converged"][0]
    assert 0.25 < conv.mean() < 0.5 and conv[C.CONVERGED_RUN[0]:C.CONVERGED_RUN[1]].all() and conv[C.CONVERGED_BLOCK[0]:C.CONVERGED_BLOCK[1]].all()
    assert C.CONVERGED_RUN[0] % 16 == 0 and C.CONVERGED_RUN[1] - C.CONVERGED_RUN[0] == 16
    assert C.CONVERGED_BLOCK[0] % TILE == 0 and C.CONVERGED_BLOCK[1] - C.CONVERGED_BLOCK[0] == TILE
    assert 0.01 < roles["two_set_few"][1].mean() < 0.06 and 0.4 < roles["two_set_many"][1].mean() < 0.5


def test_wide_rows_and_wide_transposed_rows():
    n = len(C.sequences())
    qs = list(range(n))
    rlen = np.array(S.window_lengths(_lens(), qs, 2 ** 32))
    q = np.arange(n)
    col_tiles = np.where(rlen > 0, (q + rlen) // TILE - (q + 1) // TILE + 1, 0)
    assert (col_tiles >= SEEDS + 2).sum() >= 100          # two tiles feed one class of a row
    first = np.full(n, n)          # first slot whose window holds p (full shard: slot = entry)
    for x in range(n):
        if rlen[x]:
            first[x + 1:x + 1 + rlen[x]] = np.minimum(first[x + 1:x + 1 + rlen[x]], x)
    row_tiles = np.where(first < n, (q - 1) // TILE - first // TILE + 1, 0)
    assert (row_tiles >= SEEDS + 2).sum() >= 100          # ... and of a column


def test_row_shapes():
    n = len(C.sequences())
    qs = list(range(n))
    full = np.array(S.window_lengths(_lens(), qs, 2 ** 32))
    assert (full == 0).sum() >= 3 and (full[:C.N_MAIN] == 0).sum() == 1          # the last of every group; the loner
    for depth in (300, 37):
        cut = np.array(S.window_lengths(_lens(), qs, depth))
        assert ((cut == depth) & (full > depth)).sum() >= 1000
    q = np.arange(n)
    inside = (full > 0) & ((q + 1) % 16 != 0) & ((q + 1 + full) % 16 != 0)          # begins and ends inside a chunk
    assert inside.sum() >= 1000
    one_chunk = (full > 0) & ((q + 1) // 16 == (q + full) // 16)
    assert one_chunk.sum() >= 5          # ... the same chunk


def test_byte_values():
    seen = set()
    raw_above = 0
    B = C.bound_matrix()
    for q, p, b, _, _ in _windows("uniform", 2 ** 32):
        seen.update(b.tolist())
        raw_above += int((B[q, p] > 255).sum())
    assert HUB in seen and HUB + 1 in seen
    assert any(128 <= v < 255 for v in seen)
    assert 255 in seen and raw_above >= 100          # saturated from a raw bound above 255
    assert C.TIE_BOUND in seen


def test_families_are_tuned():
    B = C.bound_matrix()
    plan = C.family_plan()
    assert {k for k, _, _ in plan} == {"row_chunk", "row_tile", "row_class", "col_chunk", "col_tile", "col_class"}
    for kind, a, sats in plan:
        assert all(B[a, p] == C.TIE_BOUND for p in sats), (kind, a)
        assert all(p > a for p in sats) if kind.startswith("row") else all(p < a for p in sats)
        x, y = sats
        if kind.endswith("chunk"):
            assert x // 16 == y // 16
        elif kind.endswith("tile"):
            assert x // 16 != y // 16 and x // TILE == y // TILE
        else:
            assert x // TILE != y // TILE and (x // TILE) % SEEDS == (y // TILE) % SEEDS


def test_row_ties_and_the_lower_index_wins():
    """the class minimum of a row attained twice in a chunk, in two chunks of a tile, in two tiles of a class: by design (the families'
    small bound) and among the unrelated sequences"""
    T = _tables("uniform", "full", 2 ** 32)
    designed, natural = set(), set()
    for q, p, b, ok, _ in _windows("uniform", 2 ** 32):
        for c in range(SEEDS):
            sel = ok & ((p // TILE) % SEEDS == c)
            if not sel.any():
                assert T["rowmin"][q][c] == ONES
                continue
            m = int(b[sel].min())
            at = p[sel & (b == m)]
            assert T["rowmin"][q][c] == (m << 32) | (int(at[0]) - q - 1)
            (designed if m == C.TIE_BOUND else natural).update(_tie_kinds(at))
    # (lengths ascend with the column: unrelated sequences of a later tile have larger bounds, so two tiles tie by design only)
    assert designed == {"chunk", "tile", "class"} and natural >= {"chunk", "tile"}


def test_column_ties_and_the_lower_index_wins():
    T = _tables("uniform", "full", 2 ** 32)
    n = len(C.sequences())
    rows = [[] for _ in range(n)]          # per entry p: (q, byte) of the rows whose window holds it
    for q, p, b, _, ok in _windows("uniform", 2 ** 32):
        for x, v in zip(p[ok].tolist(), b[ok].tolist()):
            rows[x].append((q, v))
    designed, natural = set(), set()
    for x in range(n):
        for c in range(SEEDS):
            mine = [(v, q) for q, v in rows[x] if (q // TILE) % SEEDS == c]
            if not mine:
                assert T["colmin"][x][c] == ONES
                continue
            m = min(mine)[0]
            at = np.array(sorted(q for v, q in mine if v == m))
            assert T["colmin"][x][c] == (m << 32) | int(at[0])
            (designed if m == C.TIE_BOUND else natural).update(_tie_kinds(at))
    assert designed == {"chunk", "tile", "class"} and natural >= {"chunk", "tile"}


def test_chunk_masks():
    """16-position chunks of a row (of a transposed row) whose positions are all eligible, none, some: across the role settings"""
    seen = {}
    for role in C.ROLE_NAMES:
        kinds = set()
        n = len(C.sequences())
        col_in = np.zeros((n, (n + 15) // 16), np.int32)          # per entry p and chunk of rows: window rows, eligible ones
        col_ok = np.zeros((n, (n + 15) // 16), np.int32)
        for q, p, b, ok_row, ok_col in _windows(role, 2 ** 32):
            inside = np.bincount(p // 16)
            elig = np.bincount(p // 16, weights=ok_row).astype(np.int64)
            if ((inside == 16) & (elig == 16)).any():
                kinds.add("row_all")
            if ((inside > 0) & (elig == 0)).any():
                kinds.add("row_none")
            if ((elig > 0) & (elig < inside)).any():
                kinds.add("row_some")
            col_in[p, q // 16] += 1
            col_ok[p, q // 16] += ok_col
        if ((col_in == 16) & (col_ok == 16)).any():
            kinds.add("col_all")
        if ((col_in > 0) & (col_ok == 0)).any():
            kinds.add("col_none")
        if ((col_ok > 0) & (col_ok < col_in)).any():
            kinds.add("col_some")
        seen[role] = kinds
    assert seen["uniform"] == {"row_all", "col_all"}
    assert {"row_all", "row_none", "col_all", "col_none"} <= seen["converged"]
    for role in ("two_set_few", "two_set_many"):
        assert {"row_none", "row_some", "col_none", "col_some"} <= seen[role], (role, seen[role])
    # none eligible for a whole run of 16 and a whole tile of converged entries: their rows and their columns have no minimum at all
    T = _tables("converged", "full", 2 ** 32)
    for lo, hi in (C.CONVERGED_RUN, C.CONVERGED_BLOCK):
        assert all(T["rowmin"][x] == [ONES] * SEEDS and T["colmin"][x] == [ONES] * SEEDS and T["known"][x] == [] for x in range(lo, hi))


def test_seed_pairs():
    T = _tables("uniform", "full", 2 ** 32)
    n = len(C.sequences())
    row_candidates = [sum(v != ONES for v in T["rowmin"][x]) for x in range(n)]
    assert sum(0 < k < SEEDS for k in row_candidates) >= 100          # fewer row candidates than classes
    assert sum(len(k) == 2 * SEEDS for k in T["known"]) >= 10         # a full row of the table
    assert T["known"][C.N_MAIN] == []                                   # the loner: an empty one
    col_candidates = sum(v != ONES for x in range(n) for v in T["colmin"][x])
    kept = len(T["pairs"]) - sum(row_candidates)
    assert 0 < kept < col_candidates          # column candidates that are kept, and some that are dropped as the row's own pair
    dropped = col_candidates - kept
    assert dropped >= len(C.family_plan())
    for kind, a, sats in C.family_plan():          # a family's pairs are proposed exactly once, by the row or by the column
        for p in sats:
            lo, hi = min(a, p), max(a, p)
            assert T["pairs"].count((lo, hi)) == 1 and (hi in T["known"][lo]) != (lo in T["known"][hi])
        lo, hi = min(a, sats[0]), max(a, sats[0])          # the tie's lower end: the row's own candidate, so its column's is dropped
        if kind.startswith("row"):
            assert hi in T["known"][lo]
    # the merged column classes propose fewer pairs, never more
    counts = [len(_tables("uniform", "full", 2 ** 32, c)["pairs"]) for c in (1, 2)] + [len(T["pairs"])]
    assert counts[0] < counts[1] < counts[2]
    assert len(T["pairs"]) <= 2 * SEEDS * n and all(a < b for a, b in T["pairs"])


def test_sharded_and_cut_settings_still_have_seed_pairs():
    """every setting the GPU test crosses proposes pairs from rows and from columns (no setting is vacuous)"""
    for role, shard_name, depth, classes in C.SETTINGS:
        T = _tables(role, shard_name, depth, classes)
        from_rows = sum(v != ONES for r in T["rowmin"] for v in r)
        assert from_rows > 100 and len(T["pairs"]) > from_rows, (role, shard_name, depth, classes)
