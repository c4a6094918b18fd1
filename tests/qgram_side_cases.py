"""A designed set for the side outputs of the bound kernel (hub scores, row / column minima) and the seed pairs made of them
(tests/test_gpu_qgram_seed_tables.py compares the device with tests/qgram_seed_ref.py on it, tests/test_qgram_side_cases.py asserts on
the CPU that the set still sits where it was built to sit).  Fixed seeds, numpy only, no library load.

The set, in store order (lengths ascend):
  main group   N_MAIN sequences of 300 .. 340 bases, all within 63 of each other: every window runs to the end of the group, so the first
               rows span seven column tiles and the last entries' transposed rows seven row tiles (two tiles feed one class, both ways), and
               entries around 1 000 have four classes of columns behind them AND four classes of rows in front (a full row of the table of
               the seed pairs needs both: that sets the size of the group).  Unrelated pairs of these lengths have bounds of 32 .. 37: the
               hub bound 36 and 37 both occur, and so do ties of a class minimum without any design.
  families     inside the main group: an anchor and two satellites, copies of the anchor a few spaced substitutions apart and cut or
               extended to their position's length, tuned (by the restatement of the bound) to the SAME small bound.  Row families put
               the satellites behind the anchor -- in one 16-column chunk, in two chunks of one tile, in two tiles of one class --, column
               families in front of it in the same three ways.  The anchor's row (column) proposes the satellite whose column (row)
               proposes the anchor: the candidates that are dropped as doubles.
  loner        one sequence of 800 bases: no window, in no window
  long group   LONG_A unrelated sequences of about 1 500 bases (bounds of about 147: the high bit of a bound byte)
  longer group LONG_B unrelated sequences of about 3 100 bases (bounds above 255: the byte saturates)"""
import functools

import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
N_MAIN = 1563          # not a multiple of 16: the windows of the main group end inside a chunk
LONG_A, LONG_B = 19, 21
TIE_BOUND = 6          # the bound every satellite is tuned to
FAMILIES = 36
CONVERGED_RUN = (1040, 1056)          # a whole 16-entry chunk of converged entries
CONVERGED_BLOCK = (512, 768)          # a whole 256-entry tile of them

# (is_converged, is_target) settings by name: role_settings()
ROLE_NAMES = ("uniform", "converged", "two_set_few", "two_set_many")
SHARDS = {"full": (0, None, 1, 1), "cyclic0": (0, None, 512, 256), "cyclic1": (256, None, 512, 256), "small_blocks": (8, None, 24, 8), "cut": (256, -100, 512, 256)}
DEPTHS = (2 ** 32, 300, 37)


def _random(rng, n):
    return BASES[rng.integers(0, 4, n)]


def main_length(i):
    return 300 + (i * 41) // N_MAIN


def _satellite(anchor, length, k, variant, rng):
    """the anchor cut or extended (random tail) to `length`, with k substitutions 12 bases apart from position 20 + variant on
    (a family's second satellite takes variants from 100 on: the two never get the same substitutions)"""
    y = anchor[:length].copy() if length <= len(anchor) else np.concatenate([anchor, _random(rng, length - len(anchor))])
    for j in range(k):
        at = 20 + variant + 12 * j
        y[at] = BASES[(int(np.flatnonzero(BASES == y[at])[0]) + 1 + j % 3) % 4]
    return y


def _tuned_satellite(anchor, length, first_variant, rng):
    """a satellite whose bound against the anchor is exactly TIE_BOUND (restatement of the bound, tests/qgram_ref.py)"""
    import qgram_ref as R
    pa = R.profile(anchor.tobytes().decode())
    for k in range(0, TIE_BOUND + 1):
        for variant in range(first_variant, first_variant + 8):
            y = _satellite(anchor, length, k, variant, rng)
            if R.bound(pa, R.profile(y.tobytes().decode())) == TIE_BOUND:
                return y
    raise AssertionError("no satellite with bound %d at length %d" % (TIE_BOUND, length))


def _family(f, shift):
    """(kind, anchor, satellites) of family f, its anchor moved by `shift` chunks away from the end it starts from"""
    way = f % 3
    if f % 6 < 3:          # row family: satellites behind the anchor
        a = 19 + 37 * f + 16 * shift
        c0 = (a // 16 + 1) * 16          # the chunk behind the anchor's
        if way == 0:
            sats = (c0 + 3, c0 + 9)
        elif way == 1:
            t0 = (a // 256 + 1) * 256          # the tile behind the anchor's: both chunks inside it
            sats = (t0 + 16 * (1 + f // 3 % 6) + 5, t0 + 16 * (9 + f // 3 % 6) + 2)
        else:
            sats = (c0 + 7, c0 + 7 + 1024)
        kind = "row_" + ("chunk", "tile", "class")[way]
    else:                  # column family: satellites in front of the anchor
        a = N_MAIN - 8 - 37 * (f - 3) - 16 * shift
        c0 = (a // 16 - 1) * 16
        if way == 0:
            sats = (c0 + 4, c0 + 11)
        elif way == 1:
            t0 = (a // 256 - 1) * 256
            sats = (t0 + 16 * (1 + f // 3 % 6) + 1, t0 + 16 * (9 + f // 3 % 6) + 6)
        else:
            sats = (c0 + 5 - 1024, c0 + 5)
        kind = "col_" + ("chunk", "tile", "class")[way]
    if not all(0 <= x < N_MAIN for x in sats):          # no room for a second tile of the class: a chunk family instead
        sats = (c0 + 2, c0 + 13)
        kind = kind[:4] + "chunk"
    return kind, a, sats


def family_plan():
    """[(kind, anchor position, (satellite positions))]: kind = row / col + chunk / tile / class; no position is used twice"""
    plan, used = [], set()
    for f in range(FAMILIES):
        for shift in range(8):
            kind, a, sats = _family(f, shift)
            where = (a,) + sats
            if all(0 <= x < N_MAIN for x in where) and not used.intersection(where):
                break
        else:
            raise AssertionError("no room for family %d" % f)
        used.update(where)
        plan.append((kind, a, sats))
    return plan


@functools.lru_cache(maxsize=None)
def sequences():
    """the set in store order"""
    rng = np.random.default_rng(20261)
    seqs = [_random(rng, main_length(i)) for i in range(N_MAIN)]
    for kind, a, sats in family_plan():
        for i, p in enumerate(sats):
            seqs[p] = _tuned_satellite(seqs[a], main_length(p), 100 * i, rng)
    seqs.append(_random(rng, 800))
    seqs += [_random(rng, 1500 + 2 * i) for i in range(LONG_A)]
    seqs += [_random(rng, 3100 + 2 * i) for i in range(LONG_B)]
    out = [s.tobytes().decode() for s in seqs]
    assert all(len(x) <= len(y) for x, y in zip(out, out[1:])) and len(set(out)) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def bound_matrix():
    """the restated bound of every pair of the set (tests/qgram_ref.py), computed once per process and shared: do not write to it"""
    import qgram_ref as R
    B = R.bound_matrix(sequences())
    B.setflags(write=False)
    return B


def role_settings(n):
    """name -> (is_converged, is_target), each None or uint8[n]"""
    rng = np.random.default_rng(20262)
    conv = (rng.random(n) < 0.30).astype(np.uint8)
    conv[CONVERGED_RUN[0]:CONVERGED_RUN[1]] = 1
    conv[CONVERGED_BLOCK[0]:CONVERGED_BLOCK[1]] = 1
    few = (rng.random(n) < 0.03).astype(np.uint8)
    many = (rng.random(n) < 0.45).astype(np.uint8)
    return {"uniform": (None, None), "converged": (conv, None), "two_set_few": (None, few), "two_set_many": (None, many)}


def shard(name, n):
    """(q_begin, q_end, q_stride, q_block) of a named shard for a set of n entries"""
    b, e, stride, block = SHARDS[name]
    return (b, n if e is None else n + e, stride, block)


# (roles, shard, depth, nn_seed_classes or None): every role setting on the full and a block-cyclic shard, every shard and every depth
# with the uniform and a non-uniform role setting, the merged column classes forced on the single-rank shard
SETTINGS = tuple(
    [(r, "full", 2 ** 32, None) for r in ROLE_NAMES] +
    [(r, "cyclic1", 2 ** 32, None) for r in ROLE_NAMES] +
    [(r, s, 2 ** 32, None) for s in ("cyclic0", "small_blocks", "cut") for r in ("uniform", "converged")] +
    [("two_set_many", "small_blocks", 2 ** 32, None)] +
    [(r, "full", d, None) for d in (300, 37) for r in ("uniform", "converged")] +
    [("converged", "cyclic0", 300, None), ("uniform", "small_blocks", 37, None)] +
    [(r, "full", 2 ** 32, c) for c in (1, 2) for r in ("uniform", "converged")])
