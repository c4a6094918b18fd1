"""GPU: the main pass does not align again the pairs its seed pass has settled (the model: tests/test_seed_known_model.py).

`nn_seed_skip=0` is the search as it was -- every flat pair aligned, the settled ones only counted -- so a call with it and a call
without must agree bit for bit on bounds and graph and on every counter of the filters, and differ by exactly `pairs_seed_known` in what
the pair-per-lane launch ran.  The sets are small (about 1 500 reads of 300 - 600 bases in 3 isoforms): bounds, lists, both passes of the
block filter and the pair-per-lane launch all run on them, and the variants cross every kernel that makes flat pairs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SAME = ("pairs_prefiltered", "pairs_block_rejected", "pairs_lanes", "pairs_seed_known")          # no function of a race on any path
SAME_FLAT = SAME + ("pairs_evaluated",)                                                           # ... nor this one while no table launch runs


def reads(n_reads, seed, length=450):
    from isocon_amd import synth
    seqs = sorted(dict.fromkeys(synth.make_reads(n_reads, length, 3, seed=seed)[1]), key=len)
    if len(seqs) % 64 == 0:          # (never a multiple of the wave or of the bound matrix' tile)
        seqs = seqs[:-1]
    assert len(seqs) % 64 and len(seqs) % 256
    return seqs


def graph(st, monkeypatch, variant="", **kw):
    if variant:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
    else:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    try:
        return st.nn_graph(**kw)
    finally:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)


def same_graph(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a[:3], b[:3]))


def check_pair_of_calls(skip, count, counters):
    """skip: the default call; count: the same call with nn_seed_skip=0"""
    assert same_graph(skip, count)
    s, c = skip[3], count[3]
    print({k: (s[k], c[k]) for k in SAME_FLAT + ("pairs_lanes_aligned",)})
    for k in counters:
        assert s[k] == c[k], k
    assert s["pairs_seed_known"] > 0
    assert s["pairs_lanes_aligned"] == s["pairs_lanes"] - s["pairs_seed_known"]
    assert c["pairs_lanes_aligned"] == c["pairs_lanes"]
    return s


@pytest.fixture(scope="module")
def store():
    from isocon_amd.store import SeqStore
    seqs = reads(1500, 4101)
    assert 1200 < len(seqs) <= 1500 and 250 < len(seqs[0]) and len(seqs[-1]) < 700
    st = SeqStore(seqs)
    yield seqs, st
    st.close()


def test_skip_against_count(store, monkeypatch):
    from oracle import oracle as O
    seqs, st = store
    skip, count = graph(st, monkeypatch), graph(st, monkeypatch, "nn_seed_skip=0")
    s = check_pair_of_calls(skip, count, SAME_FLAT)
    assert s["pairs_lanes_aligned"] > 0
    # every stage ran: bounds, lists, the filter, one pair per lane (and no table launch: the counters above are all deterministic)
    assert s["bound_tiles"] > 0 and s["pairs_prefiltered"] > 0 and s["pairs_block_rejected"] > 0 and s["pairs_lanes"] == s["pairs_evaluated"] > 0
    assert same_graph(graph(st, monkeypatch, "nn_seed_skip=count"), count)
    best, row_ptr, cols, _ = skip
    packed, conv = O.pack(seqs), np.zeros(len(seqs), np.uint8)
    for i in np.random.default_rng(5).choice(len(seqs), 40, replace=False).tolist():
        rp, c, e, _ = O.nn_1set(seqs, conv, i, 1, packed=packed)
        assert cols[row_ptr[i]:row_ptr[i + 1]].tolist() == c.tolist() and (e == best[i]).all(), i


@pytest.mark.parametrize("variant", ["nn_table_chunks=0", "nn_no_block_filter", "nn_no_block_filter,nn_table_chunks=0", "nn_filter_one_pass", "nn_filter_one_pass,nn_table_chunks=0"])
def test_every_kernel_that_makes_flat_pairs(store, variant, monkeypatch):
    """the list builder's remainders alone (no filter), the filter's flat output with and without its second pass, and the chunks converted
    to pairs or -- nn_table_chunks=0 -- run as tables"""
    seqs, st = store
    default = graph(st, monkeypatch)
    skip, count = graph(st, monkeypatch, variant), graph(st, monkeypatch, variant + ",nn_seed_skip=0")
    check_pair_of_calls(skip, count, SAME if "nn_table_chunks=0" in variant else SAME_FLAT)
    assert same_graph(skip, default)


def test_an_entry_whose_only_neighbour_is_its_seed(store, monkeypatch):
    """one close pair planted among the reads: two copies of a random sequence, three edits apart, far from every read -- the pair has the
    smallest bound of both its rows (a seed), is the one pair of its owner in the main pass (a flat pair) and the only edge of both rows"""
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    seqs, _ = store
    rng = np.random.default_rng(11)
    x = "".join("ACGT"[i] for i in rng.integers(0, 4, 431))
    y = x[:100] + ("A" if x[100] != "A" else "C") + x[101:250] + x[251:400] + "G" + x[400:]          # a substitution, a deletion, an insertion
    planted = sorted(dict.fromkeys(seqs[:900] + [x, y]), key=len)
    ix, iy = planted.index(x), planted.index(y)
    st = SeqStore(planted)
    try:
        skip, count = graph(st, monkeypatch), graph(st, monkeypatch, "nn_seed_skip=0")
    finally:
        st.close()
    check_pair_of_calls(skip, count, SAME_FLAT)
    best, row_ptr, cols, _ = skip
    assert cols[row_ptr[ix]:row_ptr[ix + 1]].tolist() == [iy] and cols[row_ptr[iy]:row_ptr[iy + 1]].tolist() == [ix] and best[ix] == best[iy] == 3
    conv = np.zeros(len(planted), np.uint8)
    for i in (ix, iy):
        rp, c, e, _ = O.nn_1set(planted, conv, i, 1)
        assert c.tolist() == cols[row_ptr[i]:row_ptr[i + 1]].tolist() and (e == best[i]).all()


def test_a_set_whose_every_edge_is_a_seed(monkeypatch):
    """unrelated random sequences, each with one copy a few edits away: every nearest neighbour is a seed pair, and what reaches the flat pairs
    of the main pass is settled (the pair-per-lane launch is left with little or nothing); all rows against the reference loop"""
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    rng = np.random.default_rng(12)
    seqs = []
    for _ in range(150):
        x = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(380, 420))))
        p, q = sorted(rng.integers(5, len(x) - 5, 2).tolist())
        seqs += [x, x[:p] + x[p + 1:q] + "T" + x[q:]]
    seqs = sorted(dict.fromkeys(seqs), key=len)
    st = SeqStore(seqs)
    try:
        skip, count = graph(st, monkeypatch), graph(st, monkeypatch, "nn_seed_skip=0")
    finally:
        st.close()
    s = check_pair_of_calls(skip, count, SAME_FLAT)
    assert s["pairs_seed_known"] >= len(seqs) // 2
    rp, c, e, _ = O.nn_1set(seqs, np.zeros(len(seqs), np.uint8), 0, len(seqs))
    assert (np.asarray(rp) == skip[1]).all() and (np.asarray(c) == skip[2]).all()


def test_no_stale_table_and_the_calls_that_never_use_one(store, monkeypatch):
    """a smaller store behind a larger one (the table's buffer is the larger call's), then the calls that run without the table: reads
    against candidates and a search with converged entries"""
    from isocon_amd.store import SeqStore
    seqs, st = store
    big = graph(st, monkeypatch)
    small_seqs = reads(500, 4102)
    st2 = SeqStore(small_seqs)
    try:
        skip, count = graph(st2, monkeypatch), graph(st2, monkeypatch, "nn_seed_skip=0")
    finally:
        st2.close()
    check_pair_of_calls(skip, count, SAME_FLAT)
    assert same_graph(graph(st, monkeypatch), big)
    # (what the public functions send when nothing has converged -- an array of zeros -- is the ordinary search)
    zeros = graph(st, monkeypatch, is_converged=np.zeros(len(seqs), np.uint8))
    assert same_graph(zeros, big) and zeros[3]["pairs_seed_known"] == big[3]["pairs_seed_known"] > 0
    rng = np.random.default_rng(13)
    is_target = (rng.random(len(seqs)) < 0.45).astype(np.uint8)          # many candidates: bounds, seeds and lists as in the 1-set search
    assert is_target.sum() > 512
    conv = (rng.random(len(seqs)) < 0.3).astype(np.uint8)
    for kw in ({"is_target": is_target}, {"is_converged": conv}):
        a, b = graph(st, monkeypatch, **kw), graph(st, monkeypatch, "nn_seed_skip=0", **kw)
        assert same_graph(a, b) and len(a[2]) > 0
        for g in (a, b):
            assert g[3]["pairs_seed_known"] == 0 and g[3]["pairs_lanes_aligned"] == g[3]["pairs_lanes"] > 0
        for k in SAME_FLAT:
            assert a[3][k] == b[3][k], k
