"""GPU: the launch shapes of the 64-row phase (isocon_amd/csrc/nn_scan_shape.hpp, nn_main.inc) that no other test names, at the smallest
sizes that reach them -- the length of the longest sequence selects the kernel and its waves per workgroup.  Each against the oracle loop."""
import numpy as np
import pytest

from conftest import Params, ordered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def few_errors_3kb():
    """1 200 reads of 3 kb with 0.6 % errors, and their graph by the default path (block filter, survivors one per lane).  Two thirds of the
    nearest-neighbour distances are at most 31; the isoforms have hundreds of reads each, so that without the block filter some owners keep
    the 256 pairs (NN_LIST_MIN) of either class that a table needs -- 300 reads, as first planned, launched no table there."""
    from isocon_amd import synth
    from isocon_amd.store import SeqStore
    accs, seqs, _ = synth.make_reads(1200, 3000, 3, seed=515, profile=dict(synth.CCS_PROFILE, rate=0.006))
    seqs = sorted(dict.fromkeys(seqs), key=len)
    assert 2880 < len(seqs[-1]) <= 9216
    st = SeqStore(seqs)
    yield seqs, st, st.nn_graph()
    st.close()


@pytest.mark.parametrize("tables", ["nn_table_chunks=0,nn_list_min=16", "nn_no_block_filter"])
def test_16_wave_table_launches_of_both_classes(monkeypatch, few_errors_3kb, tables):
    """Longest sequence above 2 880 bases: neither the 64-row nor the 32-row table fits three workgroups per CU, both classes launch
    with 16 waves and a raised LDS limit.  The graph is the default path's, and the rows of some reads are the reference loop's."""
    from oracle import oracle as O
    seqs, st, default = few_errors_3kb
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", tables)
    best, row_ptr, cols, stats = st.nn_graph()
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
    print(tables, {k: stats[k] for k in ("tiles", "narrow_columns", "cells_columns", "pairs_narrow", "pairs_lanes", "scan_launches")})
    assert stats["tiles"] > 0 and stats["narrow_columns"] > 0 and stats["cells_columns"] > stats["narrow_columns"], stats
    assert all((x == y).all() for x, y in zip((best, row_ptr, cols), default[:3]))
    packed = O.pack(seqs)
    conv = np.zeros(st.n, np.uint8)
    for i in list(range(0, st.n, 41)) + [st.n - 1]:
        rp, c, e, _ = O.nn_1set(seqs, conv, i, 1, packed=packed)
        assert list(cols[row_ptr[i]:row_ptr[i + 1]]) == list(c[rp[0]:rp[1]]) and (rp[1] == rp[0] or best[i] == e[rp[0]]), i


def test_16_wave_tile_synchronous_kernel_on_long_reads():
    """Longest sequence between 9 217 and 10 048 bases: too long for the lane-refill kernel's table, short enough for the 160 KB table of
    k_nn_scan_lds<16> -- without the nn_tiles variant."""
    from isocon_amd import nearest_neighbor_graph as NNG
    from isocon_amd import synth
    from oracle import oracle as O
    accs, seqs, _ = synth.make_reads(36, 9500, 3, seed=12)
    assert 9300 <= max(len(s) for s in seqs) <= 10000
    S = dict(zip(accs, seqs))
    g_gpu, _ = NNG.compute_nearest_neighbor_graph(S, set(), Params(1))
    g_cpu, _ = O.compute_nearest_neighbor_graph(S, set(), Params(1))
    assert ordered(g_gpu) == ordered(g_cpu)


def test_2set_with_many_candidates_16_wave_form(monkeypatch):
    """Reads against more than 512 candidates, longest sequence above 2 784 bases: the 16-wave form of the bounds-and-lists path and, under
    nn_no_qgram, of the unlisted launch that is left of it.  The issue that asked for this case wanted about 700 reads with every 5th
    unique sequence a candidate AND more than 512 candidates, which cannot both hold: here every 5th unique sequence is a read and the
    others are candidates (560 of 700; 2 700 reads with every 5th a candidate cost the oracle 20 s)."""
    from isocon_amd import nearest_neighbor_graph as NNG
    from isocon_amd import synth
    from oracle import oracle as O
    accs, seqs, _ = synth.make_reads(700, 3000, 3, seed=44)
    uniq = list(dict(zip(seqs, accs)).items())
    X = {a: s for k, (s, a) in enumerate(uniq) if k % 5 == 0}
    C = {"c_" + a: s for k, (s, a) in enumerate(uniq) if k % 5 != 0}
    assert len(C) > 512 and 2784 < max(len(s) for s in seqs) <= 9216
    g_cpu = O.compute_2set_nearest_neighbor_graph(X, C, Params(1))
    g_gpu = NNG.compute_2set_nearest_neighbor_graph(X, C, Params(1))
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nn_no_qgram=1")
    g_plain = NNG.compute_2set_nearest_neighbor_graph(X, C, Params(1))
    assert ordered(g_gpu) == ordered(g_plain)
    assert ordered(g_gpu) == ordered(g_cpu) and len(g_cpu) == len(X)
