"""GPU: the pair-per-lane kernel with its match vectors from the lanes' LDS tables (csrc/ed_lanes.hpp, ed_lanes_core.hpp EqFromTable; the
lane-level routine on the CPU: tests/test_lanes_eq_table_core.py).

k_ed_lanes<false> through isocon_ed_pairs with ISOCON_DEBUG_VARIANT=ed_lanes=1 (every pair in that kernel): pairs of the lengths around
the 32-column blocks and the 96-position window with the thresholds at the band's edges, each pair with two sequences of its own and
the pairs in random order, so that a wave holds different (m, n, k), lanes in the fast and in the boundary path, lanes that stop early
or never run (|m - n| > k, an empty sequence) next to pairs of 2 - 3 kb, and a last wave that is not full.  (The entry point refuses an
index of 0xffffffff, so the lanes without a pair are the ones behind the last pair here and the lists' gaps in the search below.)

k_ed_lanes<true> through the nearest-neighbour search of a small read set, seeds and main pass, with and without the block filter: every
row against the reference loop."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257)
KS = (0, 1, 31, 32, 62, 63)


def _rs(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _derive(rng, x, n, subs):
    """a sequence of length n out of x: random deletions or insertions, then `subs` substitutions"""
    y = list(x)
    while len(y) > n:
        del y[rng.randrange(len(y))]
    while len(y) < n:
        y.insert(rng.randrange(len(y) + 1), rng.choice("ACGT"))
    for _ in range(subs):
        p = rng.randrange(len(y))
        y[p] = rng.choice([c for c in "ACGT" if c != y[p]])
    return "".join(y)


def test_pairs_of_every_block_and_window_length(monkeypatch):
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    rng = random.Random(4711)
    cases = []
    for m in GRID:
        for n in GRID:
            for k in KS:
                if abs(m - n) <= k:
                    cases.append((m, n, k))
    assert len(cases) > 300
    pairs = []
    while len(pairs) < 1480:
        m, n, k = cases[len(pairs) % len(cases)] if len(pairs) < 2 * len(cases) else rng.choice(cases)
        room = k - abs(m - n)
        x = _rs(rng, m)
        pairs.append((x, _derive(rng, x, n, rng.choice([0, room // 2, room, room + 1, room + 3])) if rng.random() < 0.9 else _rs(rng, n), k))
    for m, n, k in ((40, 90, 31), (129, 64, 63), (1, 33, 31), (257, 200, 32), (0, 20, 63), (5, 0, 7), (0, 0, 0)):          # lanes that never run
        for _ in range(3):
            pairs.append((_rs(rng, m), _rs(rng, n), k))
    for L, e, k in ((2000, 10, 63), (2500, 40, 62), (3000, 63, 63), (3000, 70, 63), (2200, 0, 0), (2700, 1, 1), (2048, 33, 32)):
        x = _rs(rng, L)
        pairs.append((x, _derive(rng, x, L + rng.randint(-min(k, 5), min(k, 5)), e), k))
    rng.shuffle(pairs)
    assert len(pairs) % 64 != 0 and len(pairs) > 5 * 256
    seqs, a, b, k = [], [], [], []
    for x, y, kk in pairs:
        a.append(len(seqs)); seqs.append(x)
        b.append(len(seqs)); seqs.append(y)
        k.append(kk)
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "ed_lanes=1")
    st = SeqStore(seqs)
    try:
        got = st.ed_pairs(a, b, k)
        with pytest.raises(Exception):
            st.ed_pairs([0xffffffff], [1], [5])
    finally:
        st.close()
    want = O.ed_pairs(seqs, a, b, k)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), len(seqs[a[i]]), len(seqs[b[i]]), k[i], int(want[i]), int(got[i])) for i in bad[:10]]
    within = int((want >= 0).sum())
    assert len(pairs) // 4 < within < len(pairs) - len(pairs) // 8, within


@pytest.mark.parametrize("variant", ["", "nn_no_block_filter"])
def test_search_rows_against_the_reference_loop(variant, monkeypatch):
    from isocon_amd import synth
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    seqs = sorted(dict.fromkeys(synth.make_reads(300, 200, 3, seed=977)[1]), key=len)
    assert 200 < len(seqs) <= 300
    if variant:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
    else:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    st = SeqStore(seqs)
    try:
        best, row_ptr, cols, stats = st.nn_graph()[:4]
    finally:
        st.close()
    print({key: stats[key] for key in ("pairs_lanes", "pairs_lanes_aligned", "pairs_seed_known", "pairs_evaluated", "pairs_block_rejected")})
    assert stats["pairs_seed_known"] > 0 and stats["pairs_lanes_aligned"] > 0          # the kernel ran for the seeds and in the main pass
    rp, c, e, _ = O.nn_1set(seqs, np.zeros(len(seqs), np.uint8), 0, len(seqs))
    assert (np.asarray(rp) == row_ptr).all() and (np.asarray(c) == cols).all()
    assert (np.asarray(e) == np.repeat(best, np.diff(row_ptr))).all()
