"""GPU: the scan loop of the survivor-list builder (isocon_amd/csrc/nn_list.hpp k_nn_survivors: 256 row positions per batch, four per lane,
one dword of bounds and four meta words per load) -- the row shapes, the chunks, a sharded map and the roles of a 2-set call, at the
smallest sizes that reach them.  Nothing here depends on how the loop is written: the file passes on any library that builds the same
lists (ISOCON_LIB)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _unique_by_length(seqs):
    return sorted(dict.fromkeys(seqs), key=len)


def _graph(st, variant=None, **kw):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    if variant:
        os.environ["ISOCON_DEBUG_VARIANT"] = variant
    try:
        return st.nn_graph(**kw)
    finally:
        if variant:
            if saved is None:
                del os.environ["ISOCON_DEBUG_VARIANT"]
            else:
                os.environ["ISOCON_DEBUG_VARIANT"] = saved


def _same(a, b):
    return all((x == y).all() for x, y in zip(a[:3], b[:3]))


def test_row_shapes():
    """About 700 reads of 300 bases: the first entries have transposed rows of 0, 1, 2 ... slots and the last ones own rows of ... 2, 1, 0
    columns, so rows shorter than a lane's four positions and shorter than a batch occur at both ends of the order, the long rows end
    inside a batch, and consecutive entries start their rows at every (x + 1) mod 16.  The graph is the one of the kernel's own admission
    (nn_no_list: no list builder) and the reference loop's; the bounds reject the same pairs with and without the block filter."""
    from isocon_amd import synth
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    accs, seqs, _ = synth.make_reads(700, 300, 2, seed=77)
    seqs = _unique_by_length(seqs)
    assert len(seqs) > 600
    st = SeqStore(seqs)
    try:
        g = _graph(st)
        assert g[3]["pairs_prefiltered"] > 0
        assert _same(g, _graph(st, "nn_no_list"))
        assert _graph(st, "nn_no_block_filter")[3]["pairs_prefiltered"] == g[3]["pairs_prefiltered"]
        best, row_ptr, cols = g[:3]
        packed = O.pack(seqs)
        conv = np.zeros(st.n, np.uint8)
        rows = sorted(set(range(0, 20)) | set(range(st.n - 20, st.n)) | set(range(25, st.n - 20, (st.n - 45) // 19)))[:60]
        assert len(rows) == 60
        for i in rows:
            rp, c, e, _ = O.nn_1set(seqs, conv, i, 1, packed=packed)
            assert list(cols[row_ptr[i]:row_ptr[i + 1]]) == list(c[rp[0]:rp[1]]) and (rp[1] == rp[0] or best[i] == e[rp[0]]), i
    finally:
        st.close()


# (reads, length, isoforms, seed, error rate) -> pairs_prefiltered, pairs_block_rejected, pairs_evaluated of the default path and
# pairs_block_rejected without the filter's second pass.  The figures were recorded on an MI355X from the library of the commit before
# the 256-position scan loop (64 positions per step): which pairs share a chunk decides what the filter does with them (second pass,
# table or flat pairs), so a builder that cuts its chunks elsewhere shows in the last two.
#   one_isoform: 2 600 reads of one isoform, nearest-neighbour distances 8 .. 19 -- every read is near every other; by the final
#                thresholds at least 105 entries have more than the 2 048 pairs of a chunk and the largest has 2 581 of the 2 599 there
#                are (the entry with the largest hub score owns all of its pairs), so chunks leave in the middle of a row;
#   both_classes: the same at 8 % errors, nearest-neighbour distances 24 .. 37: thresholds on both sides of 31, so an entry's pairs
#                fill both classes of the buffer (0.7 of 3.3 million evaluated pairs leave in 32-row chunks).
# Seeds chosen among a few for a rejection by the second pass in the recorded run (the second figure above the fourth).
CHUNK_CASES = {
    "one_isoform": ((2600, 300, 1, 6, 0.04), (1908726, 1198498, 270514, 1014908)),
    "both_classes": ((2600, 300, 1, 6, 0.08), (25, 66841, 3311832, 61348)),
}


def chunk_case_reads(name):
    from isocon_amd import synth
    (n, length, iso, seed, rate), _ = CHUNK_CASES[name]
    accs, seqs, _ = synth.make_reads(n, length, iso, seed=seed, profile=dict(synth.CCS_PROFILE, rate=rate))
    return _unique_by_length(seqs)


@pytest.mark.parametrize("name", sorted(CHUNK_CASES))
def test_chunks_are_the_recorded_ones(name):
    from isocon_amd.store import SeqStore
    want = CHUNK_CASES[name][1]
    st = SeqStore(chunk_case_reads(name))
    try:
        g = _graph(st)
        one_pass = _graph(st, "nn_filter_one_pass")
        got = (g[3]["pairs_prefiltered"], g[3]["pairs_block_rejected"], g[3]["pairs_evaluated"], one_pass[3]["pairs_block_rejected"])
        print(name, got, "narrow", g[3]["pairs_narrow"])
        assert want is not None and want[1] > want[3], "the recorded run shows no rejection by the second pass"
        assert got == want
        assert _same(g, one_pass)
    finally:
        st.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_map(world):
    """2 and 4 ranks emulated in one process (blocks of the slot map with a stride, phases 0 .. 2 with the minimum of best[] between
    them, as dist.sharded_nn_graph): on a rank's transposed rows four consecutive slots are consecutive entries only inside a block,
    so the scan gathers its meta words where a lane's slots cross a block.  The graph equals the one-rank graph."""
    from isocon_amd import _lib, synth
    from isocon_amd.dist import protocol_steps
    from isocon_amd.store import SeqStore, nn_finalize
    accs, seqs, _ = synth.make_reads(900, 300, 2, seed=78)
    seqs = _unique_by_length(seqs)
    st = SeqStore(seqs)
    try:
        ref = _graph(st)
        n = st.n
        assert protocol_steps(0, world, n)[0][1][3] >= 4          # blocks of at least four entries: wide loads and gathers both occur
        best = np.full(n, _lib.NN_INF, np.int32)
        hits_all, filtered = [], 0
        for k in range(len(protocol_steps(0, world, n))):
            parts = []
            for r in range(world):
                phase, (qb, qe, qs, qk) = protocol_steps(r, world, n)[k]
                b = best.copy()
                if phase == 1:          # one pool for all ranks here: the rank's seed phase again, so that its matrix is the one in place
                    st.nn_partial(qb, qe, 0, np.full(n, _lib.NN_INF, np.int32), q_stride=qs, q_block=qk)
                hits, stats = st.nn_partial(qb, qe, phase, b, q_stride=qs, q_block=qk)
                filtered += stats["pairs_prefiltered"]
                hits_all.append(hits)
                parts.append(b)
            best = np.minimum.reduce(parts)
        hits = np.concatenate(hits_all)
        out = nn_finalize(n, best, hits[(hits[:, 2] >= 0) & (hits[:, 2] == best[hits[:, 0]])])
        assert filtered > 0
        assert _same(out, ref)
    finally:
        st.close()


def test_roles_of_a_2set_call():
    """About 750 sequences, one in five a read, the others candidates: a pair is a candidate of the scan only where one end queries and the other
    is a target.  Every row equals the reference loop's."""
    from isocon_amd import synth
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    accs, seqs, _ = synth.make_reads(800, 300, 2, seed=79)
    seqs = _unique_by_length(seqs)
    is_t = np.ones(len(seqs), np.uint8)
    is_t[::5] = 0
    assert is_t.sum() > 512          # (fewer candidates go through explicit tiles, without bounds and lists: nn_main.inc)
    st = SeqStore(seqs)
    try:
        best, row_ptr, cols, stats = _graph(st, is_target=is_t)
        assert stats["pairs_prefiltered"] > 0
        rp, c, e, _ = O.nn_2set(seqs, is_t, 0, st.n)
        assert (row_ptr == rp).all() and (cols == c).all()
        has = rp[1:] > rp[:-1]
        assert has.sum() > 50 and (best[has] == e[rp[:-1][has]]).all() and (row_ptr[1:][is_t == 1] == row_ptr[:-1][is_t == 1]).all()
    finally:
        st.close()
