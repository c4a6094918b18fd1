"""GPU: the reads x candidates search with a neighbor_search_depth that binds (smaller than the number of candidates), carried out on
the device round by round (isocon_amd/csrc/nn2_depth*.{hpp,inc}).  The checker is the oracle's restatement of the reference loop with
its depth rule (orc_nn_2set, NNG:341-424): every row, the order of its candidates and its distance."""
import os
import random
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import Params, g19, ordered

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _b_max():
    with open(os.path.join(ROOT, "isocon_amd", "csrc", "nn2_depth_core.hpp")) as f:
        return int(re.search(r"NN2_B_MAX\s*=\s*(\d+)", f.read()).group(1))


def _oracle_rows(seqs, is_t, depth, threads=16):
    """(best, row_ptr, cols, edlib calls) of the reference loop over the whole list; slices of rows on several threads (the oracle's C
    routines keep no state and ctypes releases the interpreter lock)"""
    from oracle import oracle as O
    n = len(seqs)
    packed = O.pack(seqs)
    step = max(1, min(500, (n + threads - 1) // threads))
    jobs = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda j: O.nn_2set(seqs, is_t, j[0], j[1] - j[0], depth, packed=packed), jobs))
    best = np.full(n, -1, np.int32)
    row_ptr = np.zeros(n + 1, np.int64)
    cols, calls = [], 0
    for (lo, hi), (rp, c, e, k) in zip(jobs, parts):
        rp = np.asarray(rp, dtype=np.int64)
        row_ptr[lo + 1:hi + 1] = row_ptr[lo] + rp[1:]
        has = rp[1:] > rp[:-1]
        best[lo:hi][has] = np.asarray(e)[rp[:-1][has]]
        cols.append(np.asarray(c, dtype=np.uint32))
        calls += k
    return best, row_ptr, np.concatenate(cols) if cols else np.zeros(0, np.uint32), calls


def _check_store(seqs, is_t, depth):
    from isocon_amd.store import SeqStore
    st = SeqStore(seqs)
    try:
        best, row_ptr, cols, stats = st.nn_graph(is_target=is_t, depth=depth)
    finally:
        st.close()
    ebest, erp, ecols, calls = _oracle_rows(seqs, is_t, depth)
    bad = np.flatnonzero(np.diff(row_ptr) != np.diff(erp))
    assert len(bad) == 0, "depth %d: %d rows differ in length from the reference loop, first %s" % (depth, len(bad), bad[:5])
    assert (np.asarray(cols) == ecols).all(), "depth %d" % depth
    assert (np.asarray(best) == ebest).all(), "depth %d" % depth
    return stats, calls


def _reads_and_candidates(with_n):
    from isocon_amd import synth
    rng = random.Random(59)
    nrng = np.random.Generator(np.random.PCG64(60))
    accs, seqs, isoforms = synth.make_reads(3000, 1500, 6, 4242)
    cands = list(isoforms)
    cands += [seqs[i] for i in rng.sample(range(len(seqs)), 20)]          # copies of reads: distance 0
    prof = dict(rate=0.01, ins=0.3, dele=0.3, sub=0.4)
    for iso in isoforms:
        for _ in range(5):
            cands.append(synth.mutate(nrng, np.frombuffer(iso.encode(), np.uint8), prof).tobytes().decode())
    cands.append("".join(rng.choice("ACGT") for _ in range(1500)))          # unrelated
    cands += ["".join(rng.choice("ACGT") for _ in range(1400 + 10 * i)) for i in range(12)]          # ... and more of them: every listed depth binds
    cands = list(dict.fromkeys(cands))
    items = [(s, 0) for s in seqs] + [(c, 1) for c in cands]
    if with_n:
        def spoil(s):
            v = list(s)
            for _ in range(rng.randint(1, 3)):
                v[rng.randrange(len(v))] = "N"
            return "".join(v)
        items = [(spoil(s), t) if rng.random() < (0.3 if t else 0.02) else (s, t) for s, t in items]
    items.sort(key=lambda x: len(x[0]))
    return [s for s, _ in items], np.asarray([t for _, t in items], dtype=np.uint8)


DEPTHS = (0, 1, 2, 5, 17, 59)


@pytest.mark.parametrize("with_n", [False, True], ids=["acgt", "with_N"])
def test_store_rows_equal_reference_loop(with_n):
    """depths below the number of candidates (about 69): isocon_nn_graph used to refuse them (ISOCON_E_UNSUPPORTED).  The copy with N in
    some reads and candidates sends their pairs through the byte-wise kernel (pairs_bytes)."""
    seqs, is_t = _reads_and_candidates(with_n)
    assert max(DEPTHS) < int(is_t.sum()) <= 80          # every listed depth binds
    assert any("N" in s for s in seqs) == with_n
    for depth in DEPTHS:
        stats, calls = _check_store(seqs, is_t, depth)
        assert stats["pairs_lanes"] >= calls
        assert (stats["pairs_bytes"] > 0) == with_n, depth


@pytest.mark.parametrize("depth", [1, 8, 64])
def test_c2_public_entry_equals_oracle(depth):
    from isocon_amd import nearest_neighbor_graph as NNG
    from oracle import oracle as O
    X, C, merged, fx = g19("c2")
    assert len(X) == 5000 and depth < len(C)
    g_gpu = NNG.compute_2set_nearest_neighbor_graph(X, C, Params(1, depth))
    g_cpu = O.compute_2set_nearest_neighbor_graph(X, C, Params(16, depth))
    assert ordered(g_gpu) == ordered(g_cpu)


@pytest.mark.parametrize("which,rows", [("c2", 5000), ("c3", 50000)])
def test_unlimited_depth_through_the_walk_equals_fixture(which, rows):
    """ISOCON_DEBUG_VARIANT=nn_2set_walk sends the ordinary (unlimited) 2-set call through the round scheme: same graph as the bound-matrix path"""
    from isocon_amd import nearest_neighbor_graph as NNG
    from test_gpu_configs import _check_2set_fixture
    old = os.environ.get("ISOCON_DEBUG_VARIANT")
    os.environ["ISOCON_DEBUG_VARIANT"] = "nn_2set_walk"
    try:
        n_rows, _ = _check_2set_fixture(which)
        stats = dict(NNG.LAST_STATS)
    finally:
        if old is None:
            del os.environ["ISOCON_DEBUG_VARIANT"]
        else:
            os.environ["ISOCON_DEBUG_VARIANT"] = old
    assert n_rows == rows
    assert stats["bound_tiles"] == 0 and stats["pairs_lanes"] > 0          # (the walk builds no bound matrix)


def test_c3_depth_16_rows_and_pair_count():
    """50 000 reads x 1 030 candidates at depth 16: every row equals the reference loop, and the distances asked for stay within
    calls <= pairs <= calls + 3 (B_max + 1) reads -- speculation is wasted only in the round in which a side stops and in a read's last
    round (the all-pairs fallback this replaces asked for 5.15e7)."""
    X, C, merged, fx = g19("c3")
    seqs = [s for s, _ in merged]
    is_t = np.ascontiguousarray(fx["is_target"], dtype=np.uint8)
    n_reads = int((is_t == 0).sum())
    assert n_reads == 50000
    stats, calls = _check_store(seqs, is_t, 16)
    pairs = int(stats["pairs_lanes"])
    print("calls %d, pairs %d, rounds %d, kernel %.1f ms" % (calls, pairs, stats["scan_launches"], stats["kernel_ms"]))
    assert calls <= pairs <= calls + 3 * (_b_max() + 1) * n_reads
