"""GPU: what the epilogue of k_qgram_mm leaves beside the bound matrix -- hub scores, row and column minima -- and the seed pairs
k_qgram_seed_pairs makes of them (arrays, counter, the table the main pass trusts), read back raw by isocon_qgram_seed_tables and compared
word by word with the numpy restatement tests/qgram_seed_ref.py on the designed set tests/qgram_side_cases.py (what that set covers:
tests/test_qgram_side_cases.py).  All of these outputs are integers combined by order-free atomics: the comparison is exact equality.
The bound matrix of the set and the store are made once per module; a restatement is computed once per setting."""
import numpy as np
import pytest

import qgram_seed_ref as S
import qgram_side_cases as C

pytestmark = pytest.mark.gpu

NONE32 = S.NONE32


@pytest.fixture(scope="module")
def world():
    from isocon_amd.store import SeqStore
    seqs = C.sequences()
    st = SeqStore(seqs)
    yield {"seqs": seqs, "st": st, "lens": np.array([len(s) for s in seqs]), "B": C.bound_matrix(), "roles": C.role_settings(len(seqs))}
    st.close()


def _call(st, monkeypatch, conv, targ, shard, depth, classes):
    if classes is None:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    else:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nn_seed_classes=%d" % classes)
    try:
        return st.qgram_seed_tables(conv, targ, shard[0], shard[1], shard[2], depth, shard[3])
    finally:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)


def _first_difference(got, want):
    """(row, class) of the first differing word of two [rows, classes] tables, or None"""
    bad = np.argwhere(got != want)
    return None if len(bad) == 0 else (int(bad[0][0]), int(bad[0][1]))


def _check(world, monkeypatch, role, shard_name, depth, classes):
    st, lens, B = world["st"], world["lens"], world["B"]
    n = len(lens)
    conv, targ = world["roles"][role]
    shard = C.shard(shard_name, n)
    got = _call(st, monkeypatch, conv, targ, shard, depth, classes)
    seeds, hub, tile = got["seeds"], got["hub_bound"], got["tile"]
    assert (seeds, hub, tile) == (4, 36, 256)          # what the designed set was laid out for (tests/test_qgram_side_cases.py)
    cc = S.col_classes_of(seeds, shard[2], shard[3], classes)
    assert got["col_classes"] == cc
    want = S.seed_tables(lens, B, conv, targ, shard, depth, seeds, hub, tile, cc)
    qs, rlen = want["qs"], want["rlen"]
    where = (role, shard_name, depth, classes)
    # hub scores
    bad = np.flatnonzero(got["score"].astype(np.int64) != want["score"])
    assert len(bad) == 0, where + ("score: entry %d" % bad[0], int(got["score"][bad[0]]), int(want["score"][bad[0]]), len(bad))
    # row minima, column minima
    assert got["rowmin"].shape == (len(qs), seeds) and got["colmin"].shape == (n, seeds)
    w = np.array(want["rowmin"], dtype=np.uint64).reshape(len(qs), seeds)
    d = _first_difference(got["rowmin"], w)
    assert d is None, where + ("rowmin: slot %d (entry %d), class %d" % (d[0], qs[d[0]], d[1]), hex(int(got["rowmin"][d])), hex(int(w[d])))
    w = np.array(want["colmin"], dtype=np.uint64).reshape(n, seeds)
    d = _first_difference(got["colmin"], w)
    assert d is None, where + ("colmin: entry %d, class %d" % d, hex(int(got["colmin"][d])), hex(int(w[d])))
    # the table of the seed pairs: every entry's other ends in the order it proposed them, then none
    w = np.full((n, 2 * seeds), NONE32, dtype=np.uint32)
    for x, ends in enumerate(want["known"]):
        w[x, :len(ends)] = ends
    d = _first_difference(got["known"], w)
    assert d is None, where + ("known: entry %d, place %d" % d, int(got["known"][d]), int(w[d]))
    # the seed arrays: the multiset of the entries' pairs in no defined order, nothing behind the counter
    count = got["count"]
    assert count == len(want["pairs"]) and count <= 2 * seeds * n, where + (count, len(want["pairs"]))
    assert len(got["pa"]) == len(got["pb"]) == 2 * seeds * n
    assert (got["pa"][count:] == NONE32).all() and (got["pb"][count:] == NONE32).all()
    have = sorted(zip(got["pa"][:count].tolist(), got["pb"][:count].tolist()))
    assert have == sorted(want["pairs"]), where + ("pairs", [x for x in have if x not in set(want["pairs"])][:3], [x for x in want["pairs"] if x not in set(have)][:3])
    # ... and by themselves, without the restatement: the table names exactly the pairs of the launch (a pair in the table that the launch
    # does not hold would be a neighbour the main pass never aligns), every pair ascends, lies in its row's window and has an owned row
    table = sorted((min(x, int(y)), max(x, int(y))) for x in range(n) for y in got["known"][x] if y != NONE32)
    assert table == have, where + ("known against the seed arrays",)
    slot_of = {q: s for s, q in enumerate(qs)}
    for a, b in have:
        assert a < b and a in slot_of and b - a <= rlen[slot_of[a]], where + (a, b)
    return got, want


@pytest.mark.parametrize("role,shard_name,depth,classes", C.SETTINGS, ids=["%s-%s-%s-%s" % (r, s, "all" if d == 2 ** 32 else d, c or "auto") for r, s, d, c in C.SETTINGS])
def test_every_word_against_the_restatement(world, monkeypatch, role, shard_name, depth, classes):
    got, want = _check(world, monkeypatch, role, shard_name, depth, classes)
    if role == "uniform" and shard_name == "full":
        # every window pair within the hub bound counts once at either end
        assert int(got["score"].astype(np.int64).sum()) == 2 * want["hub_pairs"] and want["hub_pairs"] > 0


def test_the_entry_leaves_no_state_behind(world, monkeypatch):
    """a search before and after a call of the test entry: the same graph, the same settled pairs"""
    st = world["st"]
    n = len(world["lens"])
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    conv = world["roles"]["converged"][0]
    for kw in ({}, {"is_converged": conv}):
        before = st.nn_graph(**kw)
        st.qgram_seed_tables(conv, None, *C.shard("cyclic1", n)[:3], depth=300, q_block=256)
        st.qgram_seed_tables(None, world["roles"]["two_set_many"][1])
        after = st.nn_graph(**kw)
        assert all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(before[:3], after[:3]))
        assert before[3]["pairs_seed_known"] == after[3]["pairs_seed_known"]
        for k in ("pairs_prefiltered", "pairs_block_rejected", "pairs_lanes", "bound_tiles"):
            assert before[3][k] == after[3][k], k
    assert st.nn_graph()[3]["pairs_seed_known"] > 0


def test_argument_and_alphabet_errors(world):
    """as isocon_qgram_bound_matrix: a stride or block that is no shard, a set with more than four symbols"""
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    st = world["st"]
    for stride, block in ((0, 1), (4, 3), (2, 4)):
        with pytest.raises(_lib.IsoconError) as e:
            st.qgram_seed_tables(q_stride=stride, q_block=block)
        assert e.value.status == _lib.ISOCON_E_ARG
    st2 = SeqStore(sorted(["ACGTNACGTRYACGT" * 3, "ACGTACGTACGTAAAA" * 3, "ACGTKMACGTAAAACC" * 3], key=len))
    try:
        with pytest.raises(_lib.IsoconError) as e:
            st2.qgram_seed_tables()
        assert e.value.status == _lib.ISOCON_E_ALPHABET
    finally:
        st2.close()
    # no pair inside any window: every table keeps its fill
    st3 = SeqStore(["ACGT" * 10, "ACGT" * 40, "TTGCA" * 60])
    try:
        t = st3.qgram_seed_tables()
        assert t["count"] == 0 and (t["score"] == 0).all() and (t["known"] == NONE32).all() and (t["pa"] == NONE32).all() and (t["pb"] == NONE32).all()
        assert (t["rowmin"] == np.uint64(S.ONES)).all() and (t["colmin"] == np.uint64(S.ONES)).all()
    finally:
        st3.close()
