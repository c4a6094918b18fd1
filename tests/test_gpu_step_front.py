"""GPU: the front of one NN-graph step -- the profile kernel (k_qgram_profile4) also writes the block filter's 2-bit text rows, the row
layout of the transposed matrix and the fills of the seed arrays run on the side stream under it, the step starts with one launch
instead of five fills -- computes what the step computed before.

The text rows.  `store.block_bound_pairs` reads a text that it builds itself with k_build_text2, never the one a step left: what it
checks here is the packing expression both kernels share (text2_word), against a greedy 8-gram count written out below.  The rows the
profile kernel wrote are read by the step's own block filter, so they are checked through the step: its graph against the oracle, and
graph and `pairs_block_rejected` (the number of pairs the filter dropped: no function of any race, tests/test_gpu_step_schedule.py)
against the same search run as a seed phase and a main phase of `nn_partial` -- the main phase finds the bound matrix in the pool, runs
no profile kernel and has its text from k_build_text2.

Sequence counts: 1, 3 and QP_SEQS - 1, QP_SEQS, QP_SEQS + 1, 2 QP_SEQS + 1 for each of the values 4, 8 and 16 that QP_SEQS (sequences per
workgroup of the profile kernel, a compile-time constant the library does not report) may take.  Lengths: every packing edge of a text
dword (16 bases), of a plane word (64) and of a text piece (256)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests import qgram_ref as R

pytestmark = pytest.mark.gpu

EDGE_LENS = (1, 7, 8, 15, 16, 17, 23, 24, 255, 256, 257, 271, 272)
COUNTS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33)


def _edge_store(count, seed=7):
    """`count` different sequences, their lengths the edge lengths in turn: prefixes of one random sequence with one base changed"""
    rng = np.random.default_rng(seed)
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, max(EDGE_LENS)))
    seen, out = set(), []
    for i in range(count):
        L = EDGE_LENS[i % len(EDGE_LENS)]
        while True:
            p = int(rng.integers(0, L))
            s = base[:p] + "ACGT"[int(rng.integers(0, 4))] + base[p + 1:L]
            if s not in seen:
                break
        seen.add(s)
        out.append(s)
    return sorted(out, key=len)


def _read_store(seed, n, length):
    """reads of a few isoforms (chunks for the block filter) with a prefix of every edge length among them"""
    from isocon_amd import synth
    _, seqs, iso = synth.make_reads(n, length, 3, seed)
    longest = max(iso, key=len)
    return sorted(dict.fromkeys(seqs + [longest[:L] for L in EDGE_LENS]), key=len)


def block_count(owner, partner, s):
    """nn_filter.hpp in plain Python: 8-grams of `partner` at the positions 0, s, 2 s, ... of its whole 16-base words whose grams all lie
    inside it; one that occurs nowhere in `owner` counts and skips the probes that overlap it"""
    grams = {owner[i:i + 8] for i in range(len(owner) - 7)}
    words = (len(partner) - (16 - s + 8)) // 16 + 1 if len(partner) >= 16 - s + 8 else 0
    count, free = 0, 0
    for p in range(0, 16 * words, s):
        if p >= free and partner[p:p + 8] not in grams:
            count += 1
            free = p + 8
    return count


@contextmanager
def _variant(value):
    old = os.environ.get("ISOCON_DEBUG_VARIANT")
    if value:
        os.environ["ISOCON_DEBUG_VARIANT"] = value
    else:
        os.environ.pop("ISOCON_DEBUG_VARIANT", None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("ISOCON_DEBUG_VARIANT", None)
        else:
            os.environ["ISOCON_DEBUG_VARIANT"] = old


_ORACLE = {}


def _oracle(seqs):
    """(row_ptr, cols, eds) of the 1-set graph, computed once per set"""
    key = tuple(seqs)
    if key not in _ORACLE:
        from oracle import oracle as O
        n = len(seqs)
        _ORACLE[key] = O.nn_1set(seqs, np.zeros(n, np.uint8), 0, n)[:3]
    return _ORACLE[key]


def _assert_oracle(seqs, best, rp, cols):
    rpo, co, eo = _oracle(seqs)
    assert (np.asarray(rp) == rpo).all() and (np.asarray(cols) == co).all()
    for q in range(len(seqs)):
        assert (best[q] < 0 and rp[q] == rp[q + 1]) or (eo[rp[q]:rp[q + 1]] == best[q]).all(), q


def _graph(st, variant=""):
    with _variant(variant):
        best, rp, cols, stats = st.nn_graph()
    return best.copy(), rp.copy(), cols.copy(), stats


def _graph_in_phases(st):
    """the same search as seed phase, main phase and wide phase of nn_partial and the host's CSR; the main phase's statistics"""
    from isocon_amd import _lib
    from isocon_amd.store import nn_finalize
    n = st.n
    best = np.full(max(n, 1), _lib.NN_INF, np.int32)
    hits, main = [], None
    for phase in (0, 1, 2):
        h, stats = st.nn_partial(0, n, phase, best)
        hits.append(h)
        if phase == 1:
            main = stats
    return nn_finalize(n, best[:n], np.concatenate(hits)), main


def _all_pairs(n):
    a, b = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), indexing="ij")
    return a.ravel(), b.ravel()


@pytest.mark.parametrize("count", COUNTS)
def test_text_packing_against_the_greedy_count(count):
    from isocon_amd.store import SeqStore
    seqs = _edge_store(count)
    assert len(seqs) == count
    a, b = _all_pairs(count)
    st = SeqStore(seqs)
    try:
        for s in (4, 2):
            got = st.block_bound_pairs(a, b, probe_stride=s)
            want = np.array([block_count(seqs[x], seqs[y], s) for x, y in zip(a, b)], np.int32)
            assert (got == want).all(), (s, np.flatnonzero(got != want)[:8])
    finally:
        st.close()


@pytest.mark.parametrize("count", COUNTS)
def test_profiles_and_graph_of_edge_stores(count):
    """n below, at and above a multiple of every QP_SEQS: the bounds of all pairs against the lemma restated in numpy, the step's graph
    against the oracle and against the search in phases"""
    from isocon_amd.store import SeqStore
    seqs = _edge_store(count)
    st = SeqStore(seqs)
    try:
        a, b = _all_pairs(count)
        prof = [R.profile(s) for s in seqs]
        want = np.array([R.bound(prof[x], prof[y]) for x, y in zip(a, b)], np.int32)
        assert (st.qgram_bound_pairs(a, b) == want).all()
        best, rp, cols, _ = _graph(st)
        _assert_oracle(seqs, best, rp, cols)
        if count >= 2:
            (pb, prp, pcols), _ = _graph_in_phases(st)
            assert (pb == best[:count]).all() and (prp == rp).all() and (pcols == cols).all()
        best2, rp2, cols2, _ = _graph(st)          # (the pool's buffers a second time)
        assert (best2 == best).all() and (rp2 == rp).all() and (cols2 == cols).all()
    finally:
        st.close()


@pytest.fixture(scope="module")
def read_sets():
    return _read_store(61, 700, 280), _read_store(62, 450, 330)


def test_filter_reads_the_text_the_profile_kernel_wrote(read_sets):
    from isocon_amd.store import SeqStore
    seqs = read_sets[0]
    assert set(EDGE_LENS) <= {len(s) for s in seqs}
    st = SeqStore(seqs)
    try:
        best, rp, cols, stats = _graph(st)
        _assert_oracle(seqs, best, rp, cols)
        assert stats["pairs_block_rejected"] > 0 and stats["filter_kernel_ms"] > 0          # the filter ran and decided something
        (pb, prp, pcols), main = _graph_in_phases(st)
        assert main["bound_kernel_ms"] == 0          # no profile kernel in the main phase: its text is k_build_text2's
        assert main["pairs_block_rejected"] == stats["pairs_block_rejected"]
        assert (pb == best[:len(seqs)]).all() and (prp == rp).all() and (pcols == cols).all()
    finally:
        st.close()


@pytest.mark.parametrize("variant", ["", "nn_sync_uploads", "nn_no_block_filter"])
def test_stores_of_different_size_in_turn(read_sets, variant):
    """A, B (another n, another longest sequence), A again in one process: the pool's buffers, the pinned block and the side stream are
    used again with other sizes; with the side stream off and with the filter off (no text rows) the graphs are the same"""
    from isocon_amd.store import SeqStore
    sa, sb = read_sets
    assert len(sa) != len(sb)
    stores = {"a": SeqStore(sa), "b": SeqStore(sb)}
    try:
        for key in ("a", "b", "a"):
            seqs = sa if key == "a" else sb
            best, rp, cols, stats = _graph(stores[key], variant)
            _assert_oracle(seqs, best, rp, cols)
            assert (stats["pairs_block_rejected"] > 0) == (variant != "nn_no_block_filter")
    finally:
        for st in stores.values():
            st.close()
