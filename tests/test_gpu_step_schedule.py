"""GPU: the schedule of one NN-graph call -- phase timers that only record events and are resolved once, inputs filled on the device,
the nibble text built in front of the first launch that reads it, one record at the end of the 64-row phase and one download of the
CSR -- computes what the call computes with a wait after every phase (ISOCON_DEBUG_VARIANT=nn_sync_phases): the same bounds, the same
graph, the same pair counters, on every path the call can take.

`hits` -- the candidate edges the kernels recorded, stale ones included -- is no function of the input: whether a pair that ties or
beats an endpoint's bound is recorded depends on which wave reached best[] first.  Three calls of the unchanged library on the
set of the plain case gave 28928, 28379 and 28444, two with a wait after every phase 28697 and 28696.  Two calls are therefore compared
on what is fixed -- the three pair counters, the bounds and the graph -- and `hits` on its invariant: every edge of the graph was
recorded at least once.  The same holds for the pair counters of a call whose pairs go through the table kernel's own admission
(k_nn_scan_refill reads the thresholds while other waves tighten them; `nn_list_cap=1` gave pairs_prefiltered 574811 and 574881 on
one set): such calls -- the table variants and the list fallback -- are compared on bounds, graph and pairs_block_rejected, which
comes from the list builder's totals and is fixed before a table kernel runs."""
import os
import time
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("pairs_prefiltered", "pairs_block_rejected", "pairs_evaluated")
# Blocking host waits of the plain 1-set call on 2048 entries (isocon_nn_last_host_waits): the launch order of
# the main pass goes up (sets of up to 16384 entries have one), the list totals come back behind the block filter, one record ends the
# 64-row phase, one record and one download end the CSR kernels.
PLAIN_WAITS = 1 + 1 + 1 + 2


def _reads(seed, n=2048, length=300, iso=4):
    from isocon_amd import synth
    _, seqs, _ = synth.make_reads(n, length, iso, seed)
    return sorted(dict.fromkeys(seqs), key=len)


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


def _graph(seqs, variant="", **kw):
    """(best, row_ptr, cols, stats, host waits) of one call on a new store"""
    from isocon_amd.store import SeqStore
    st = SeqStore(seqs)
    try:
        with _variant(variant):
            best, rp, cols, stats = st.nn_graph(**kw)
        return best.copy(), rp.copy(), cols.copy(), stats, int(st._L.isocon_nn_last_host_waits(st._h))
    finally:
        st.close()


FIXED = ("pairs_block_rejected",)          # no function of a race on any path


def _same(a, b, counters=COUNTERS):
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    for k in counters:
        assert a[3][k] == b[3][k], (k, a[3][k], b[3][k])
    for x in (a, b):
        assert x[3]["hits"] >= len(x[2]), (x[3]["hits"], len(x[2]))


def _both(seqs, variant="", counters=COUNTERS, **kw):
    """the default schedule and the one that waits after every phase, compared; returns the default's result"""
    a = _graph(seqs, variant, **kw)
    b = _graph(seqs, (variant + "," if variant else "") + "nn_sync_phases", **kw)
    _same(a, b, counters)
    return a, b


@pytest.fixture(scope="module")
def plain():
    seqs = _reads(41)
    a, b = _both(seqs)
    return seqs, a, b


def test_plain_one_set_against_the_oracle(plain):
    from oracle import oracle as O
    seqs, (best, rp, cols, stats, _), _ = plain
    n = len(seqs)
    assert n >= 1024 and stats["pairs_evaluated"] > 0 and len(cols) > 0
    rpo, co, eo, _ = O.nn_1set(seqs, np.zeros(n, np.uint8), 0, n)
    assert (rp == rpo).all() and (cols == co).all()
    for q in range(n):
        assert (best[q] < 0 and rp[q] == rp[q + 1]) or (eo[rp[q]:rp[q + 1]] == best[q]).all()


def test_plain_host_waits_and_timers(plain):
    seqs, a, b = plain
    assert a[4] == PLAIN_WAITS, a[4]
    assert a[4] < b[4]
    from isocon_amd.store import SeqStore
    st = SeqStore(seqs)
    try:
        st.nn_graph()
        t0 = time.perf_counter()
        _, _, _, s = st.nn_graph()
        wall_ms = (time.perf_counter() - t0) * 1e3
    finally:
        st.close()
    fields = ("bound_kernel_ms", "mm_kernel_ms", "seed_kernel_ms", "list_kernel_ms", "filter_kernel_ms", "lanes_kernel_ms", "scan_kernel_ms", "narrow_kernel_ms", "kernel_ms")
    for k in fields:
        assert s[k] >= 0, (k, s[k])
    assert s["bound_kernel_ms"] > 0 and s["seed_kernel_ms"] > 0 and s["list_kernel_ms"] > 0
    assert s["bound_kernel_ms"] >= s["mm_kernel_ms"] > 0
    assert s["list_kernel_ms"] >= s["filter_kernel_ms"] > 0
    phases = s["bound_kernel_ms"] + s["seed_kernel_ms"] + s["list_kernel_ms"] + s["lanes_kernel_ms"] + s["scan_kernel_ms"]
    assert phases <= s["kernel_ms"] + 0.05, (phases, s["kernel_ms"])
    assert s["kernel_ms"] <= wall_ms, (s["kernel_ms"], wall_ms)


def test_blocking_row_layout_uploads(plain):
    """nn_sync_uploads: tile table, row offsets and row lengths in three blocking copies -- also what a call does when the side stream or
    its pinned block cannot be made"""
    seqs, a, _ = plain
    c = _graph(seqs, "nn_sync_uploads")
    _same(a, c)
    assert c[4] == PLAIN_WAITS + 3, c[4]


def test_one_set_with_converged_entries():
    seqs = _reads(42)
    conv = (np.arange(len(seqs)) % 5 == 0).astype(np.uint8)          # role flags that are no constants: the upload path
    a, _ = _both(seqs, is_converged=conv)
    assert (a[1][1:][conv == 1] == a[1][:-1][conv == 1]).all()          # a converged entry queries nothing
    assert len(a[2]) > 0


@pytest.mark.parametrize("n_targets", [600, 40])          # > 512 targets: bounds and lists; few: explicit tiles
def test_two_set(n_targets):
    seqs = _reads(43)
    targ = np.zeros(len(seqs), np.uint8)
    targ[np.random.default_rng(n_targets).choice(len(seqs), n_targets, replace=False)] = 1
    a, _ = _both(seqs, is_target=targ)
    assert len(a[2]) > 0 and (a[1][1:][targ == 1] == a[1][:-1][targ == 1]).all()


@pytest.mark.parametrize("n", [700, 0, 1, 2])          # below 1024 entries the CSR is the host's
def test_small_sets(n):
    seqs = _reads(44, n=900)[:n] if n else []
    a, _ = _both(seqs)
    assert len(a[1]) == n + 1


def test_hit_list_overflow_retry():
    seqs = _reads(45)
    ref = _graph(seqs)
    a, _ = _both(seqs, "hits_cap=64")
    _same(a, ref, counters=())
    assert ref[3]["hits"] > 64 and a[3]["hits"] > 64          # (the list did overflow; the second pass records every final hit again)
    assert a[3]["kernel_ms"] > 0 and a[3]["seed_kernel_ms"] > 0 and a[3]["bound_kernel_ms"] >= a[3]["mm_kernel_ms"] > 0


@pytest.mark.parametrize("variant", ["nn_table_chunks=0", "nn_no_block_filter"])
def test_table_launches_find_their_text(variant):
    seqs = _reads(46)
    ref = _graph(seqs)
    a, _ = _both(seqs, variant, counters=FIXED)
    _same(a, ref, counters=())
    assert a[3]["scan_kernel_ms"] > 0 and a[3]["cells_columns"] > 0          # table launches ran: they read the nibble text


def test_list_fallback():
    seqs = _reads(47)
    ref = _graph(seqs)
    a, _ = _both(seqs, "nn_list_cap=1", counters=FIXED)
    _same(a, ref, counters=())


def test_two_stores_alternately():
    from isocon_amd.store import SeqStore
    sa, sb = SeqStore(_reads(48)), SeqStore(_reads(49, n=1500, length=420))
    try:
        first = {}
        for _ in range(3):
            for key, st in (("a", sa), ("b", sb)):
                best, rp, cols, stats = st.nn_graph()
                got = (best.copy(), rp.copy(), cols.copy(), stats)
                if key not in first:
                    first[key] = got
                _same(got, first[key])
                assert stats["kernel_ms"] > 0
    finally:
        sa.close()
        sb.close()


def test_sharded_phases_equal_the_graph():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore, nn_finalize
    seqs = _reads(50)
    st = SeqStore(seqs)
    try:
        ref = st.nn_graph()
        n = st.n
        best = np.full(n, _lib.NN_INF, np.int32)
        hits_all = []
        reused = 0
        for phase in (0, 1, 2):
            parts = []
            for r in ((0, 1) if phase != 1 else (1, 0)):
                b = best.copy()
                hits, stats = st.nn_partial(r * 64, n, phase, b, q_stride=128, q_block=64)
                # the main phase that directly follows its own shard's seed phase finds the bound matrix still in place
                if phase == 1 and r == 1:
                    assert stats["bound_kernel_ms"] == 0 and stats["pairs_prefiltered"] > 0
                    reused += 1
                assert all(stats[k] >= 0 for k in stats if k.endswith("_ms"))
                hits_all.append(hits); parts.append(b)
            best = np.minimum.reduce(parts)
        assert reused == 1
        out = nn_finalize(n, best, np.concatenate(hits_all))
        assert all((x == y).all() for x, y in zip(out[:3], ref[:3]))
    finally:
        st.close()
