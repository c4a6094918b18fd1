"""GPU: the block test of the depth-limited reads x candidates search (isocon_amd/csrc/nn2_depth.hpp, k_nn2_block_reject): a listed pair
whose greedy count of disjoint 8-grams of the candidate that occur nowhere in the read exceeds its threshold is final with the -1 edlib
would return and is never aligned (the search runs it under ISOCON_DEBUG_VARIANT=nn2_block_filter).  What the kernel decides pair by
pair (isocon_nn2_block_reject) against the count of the main pass's test entry (isocon_block_bound_pairs) and exact distances; and
the search's rows and counters with the test and without it against the oracle's restatement of the reference loop (orc_nn_2set,
NNG:341-424)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTHS = (1, 5, 17)
ON = "nn2_block_filter"          # ISOCON_DEBUG_VARIANT that turns the walk's block test on (off by default: profiles/nn2set_depth.txt)


# ---- 1. per-pair decisions ------------------------------------------------------------------------------------------------------

# no gram or one; around the first dword of nnf_dwords for both strides; around a 256-base piece and its 17th dword; long
LENGTHS = [0, 5, 7, 8, 9, 21, 22, 23, 24, 25, 255, 256, 257, 271, 272, 273]
RUNS = (1, 33, 64, 65)          # a lone lane, a run as the search lists it, a full task, a run that is cut


def _noisy(rng, root, length, edits):
    v = list(root[:length + 8])
    for _ in range(edits):
        if not v:
            break
        p = rng.randrange(len(v))
        r = rng.random()
        if r < 0.4:
            v[p] = rng.choice("ACGT")
        elif r < 0.7:
            del v[p]
        else:
            v.insert(p, rng.choice("ACGT"))
    v = v[:length]
    while len(v) < length:
        v.append(rng.choice("ACGT"))
    return "".join(v)


def _pair_store():
    rng = random.Random(77)
    roots = ["".join(rng.choice("ACGT") for _ in range(640)) for _ in range(3)]
    seqs = []
    for length in LENGTHS:
        for r, root in enumerate(roots):
            seqs.append(_noisy(rng, root, length, 0 if r == 0 else max(1, length // 40)))
    for root in roots:
        seqs += [root[:600], _noisy(rng, root, 600, 6), _noisy(rng, root, 600, 40)]
    seqs += ["".join(rng.choice("ACGT") for _ in range(length)) for length in (24, 256, 272, 600, 600)]          # unrelated
    assert 55 <= len(seqs) <= 65
    return seqs


def _pair_list(n):
    """every read against 1, 33, 64 and 65 targets; neighbouring runs belong to different reads"""
    read, target = [], []
    for t in RUNS:
        for x in range(n):
            read += [x] * t
            target += [(x + 1 + 7 * j) % n for j in range(t)]          # (7 and n coprime or not: targets repeat, the read itself turns up -- all allowed)
    return np.asarray(read, np.uint32), np.asarray(target, np.uint32)


@pytest.fixture(scope="module")
def pair_case():
    from isocon_amd.store import SeqStore
    from oracle import oracle as O
    seqs = _pair_store()
    read, target = _pair_list(len(seqs))
    st = SeqStore(seqs)
    counts = {s: st.block_bound_pairs(read, target, probe_stride=s).astype(np.int64) for s in (2, 4)}
    dist = {}
    for x, y in set(zip(read.tolist(), target.tolist())):
        dist[(x, y)] = O.ed_dp(seqs[x], seqs[y])
    d = np.asarray([dist[(x, y)] for x, y in zip(read.tolist(), target.tolist())], np.int64)
    yield seqs, read, target, counts, d, st
    st.close()


def _thresholds(c):
    return [np.zeros_like(c), np.maximum(c - 1, 0), c, c + 1, np.full_like(c, 10 ** 6)]


@pytest.mark.parametrize("stride", [2, 4])
def test_per_pair_decisions(pair_case, stride):
    """out_rejected[p] == (count > k[p]) for k in {0, c - 1, c, c + 1, 10^6} on runs of 1, 33, 64 and 65 pairs, and a rejected pair's
    distance exceeds k[p].  (Fails where the entry does not exist.)"""
    seqs, read, target, counts, d, st = pair_case
    c = counts[stride]
    assert (c <= d).all()
    assert (c > 0).sum() > 1000 and (c == 0).sum() > 50          # both outcomes occur at k = 0
    n_rejected = 0
    for k in _thresholds(c):
        got = st.nn2_block_reject(read, target, k, probe_stride=stride).astype(bool)
        want = c > k
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, "stride %d: %d pairs differ, first %s" % (stride, len(bad), [(int(read[p]), int(target[p]), int(k[p]), int(c[p])) for p in bad[:5]])
        assert (d[got] > k[got]).all()
        n_rejected += int(got.sum())
    assert n_rejected > 0
    # a negative threshold marks a pair outside the planes' map: not tested
    k = np.where(np.arange(len(c)) % 3 == 0, -1, 0).astype(np.int32)
    got = st.nn2_block_reject(read, target, k, probe_stride=stride).astype(bool)
    assert (got == ((c > 0) & (k >= 0))).all()


def test_default_stride_is_the_finer_grid(pair_case):
    seqs, read, target, counts, d, st = pair_case
    assert (st.nn2_block_reject(read, target, np.zeros(len(read), np.int32)).astype(bool) == (counts[2] > 0)).all()


@pytest.mark.parametrize("stride", [2, 4])
def test_pairs_with_n_are_not_tested(pair_case, stride):
    """a copy of the store with N in some sequences: no ISOCON_E_ALPHABET, pairs with such an entry come back 0 whatever k, all others
    as on the clean store"""
    from isocon_amd.store import SeqStore
    seqs, read, target, counts, d, st = pair_case
    rng = random.Random(5)
    spoiled = [i for i in range(len(seqs)) if len(seqs[i]) >= 5 and i % 5 == 2]
    seqs_n = list(seqs)
    for i in spoiled:
        v = list(seqs_n[i])
        v[rng.randrange(len(v))] = "N"
        seqs_n[i] = "".join(v)
    has_n = np.zeros(len(seqs), bool)
    has_n[spoiled] = True
    exceptional = has_n[read] | has_n[target]
    assert 0 < exceptional.sum() < len(read)
    c = counts[stride]
    st_n = SeqStore(seqs_n)
    try:
        for k in (np.zeros_like(c), np.maximum(c - 1, 0), c):
            got = st_n.nn2_block_reject(read, target, k, probe_stride=stride).astype(bool)
            assert not got[exceptional].any()
            assert (got[~exceptional] == (c > k)[~exceptional]).all()
    finally:
        st_n.close()


def test_argument_errors(pair_case):
    from isocon_amd import _lib
    seqs, read, target, counts, d, st = pair_case
    n = len(seqs)
    k = np.zeros(3, np.int32)
    for bad_read, bad_target in (([0, n, 1], [1, 2, 3]), ([0, 1, 2], [1, 2, n])):
        with pytest.raises(_lib.IsoconError) as e:
            st.nn2_block_reject(bad_read, bad_target, k)
        assert e.value.status == _lib.ISOCON_E_ARG
    for stride in (0, 1, 3, 8):
        with pytest.raises(_lib.IsoconError) as e:
            st.nn2_block_reject([0, 1, 2], [1, 2, 3], k, probe_stride=stride)
        assert e.value.status == _lib.ISOCON_E_ARG
    assert len(st.nn2_block_reject([], [], [])) == 0


# ---- 2 - 4. rows and counters of the search ---------------------------------------------------------------------------------------

def _roles(rng, nrng, seqs, isoforms, lo, hi, with_n):
    from isocon_amd import synth
    cands = list(isoforms)
    prof = dict(rate=0.01, ins=0.3, dele=0.3, sub=0.4)
    for iso in isoforms:
        for _ in range(5):
            cands.append(synth.mutate(nrng, np.frombuffer(iso.encode(), np.uint8), prof).tobytes().decode())
    cands += [seqs[i] for i in rng.sample(range(len(seqs)), 10)]          # copies of reads: distance 0
    # unrelated ones with lengths spread over the reads' range: they lie inside the walk's window after a read has found its candidate
    cands += ["".join(rng.choice("ACGT") for _ in range(lo + (hi - lo) * i // 11)) for i in range(12)]
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


def _set(with_n):
    """800 reads of about 400 bases in 4 isoforms against about 45 candidates: the isoforms, five mutated copies of each, ten copies
    of reads and a dozen unrelated sequences"""
    from isocon_amd import synth
    rng = random.Random(91)
    nrng = np.random.Generator(np.random.PCG64(92))
    accs, seqs, isoforms = synth.make_reads(800, 400, 4, 2024)
    lens = [len(s) for s in seqs]
    return _roles(rng, nrng, seqs, isoforms, min(lens), max(lens), with_n)


def _short_set():
    """the same roles on sequences of 3 to 7 bases: no target holds an 8-gram"""
    rng = random.Random(93)
    isoforms = ["".join(rng.choice("ACGT") for _ in range(length)) for length in (4, 5, 6, 7)]

    def noisy(s):
        v = list(s)
        if rng.random() < 0.5:
            v[rng.randrange(len(v))] = rng.choice("ACGT")
        if rng.random() < 0.3 and len(v) > 3:
            del v[rng.randrange(len(v))]
        elif rng.random() < 0.3 and len(v) < 7:
            v.insert(rng.randrange(len(v) + 1), rng.choice("ACGT"))
        return "".join(v)
    seqs = [noisy(rng.choice(isoforms)) for _ in range(800)]
    cands = list(isoforms) + [noisy(iso) for iso in isoforms for _ in range(5)] + [seqs[i] for i in rng.sample(range(800), 10)]
    cands += ["".join(rng.choice("ACGT") for _ in range(3 + i % 5)) for i in range(12)]
    items = [(s, 0) for s in seqs] + [(c, 1) for c in cands]
    items.sort(key=lambda x: len(x[0]))
    assert 3 <= len(items[0][0]) and len(items[-1][0]) <= 7
    return [s for s, _ in items], np.asarray([t for _, t in items], dtype=np.uint8)


_ORACLE = {}
# (listed pairs, of them with count > k) of _set(False) per depth, from the CPU round scheme and the Python count (see the test's docstring)
EXPECTED = {1: (818, 0), 5: (3968, 1714), 17: (9228, 5431)}


def _reference(name, seqs, is_t, depth):
    """rows of the reference loop, computed once per (set, depth)"""
    from test_gpu_nn2set_depth import _oracle_rows
    if (name, depth) not in _ORACLE:
        _ORACLE[(name, depth)] = _oracle_rows(seqs, is_t, depth)
    return _ORACLE[(name, depth)]


def _graph(seqs, is_t, depth, monkeypatch, variant=None):
    from isocon_amd.store import SeqStore
    if variant:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
    else:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    st = SeqStore(seqs)
    try:
        best, row_ptr, cols, stats = st.nn_graph(is_target=is_t, depth=depth)
    finally:
        st.close()
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    return np.asarray(best), np.asarray(row_ptr).astype(np.int64), np.asarray(cols), stats


def _assert_rows(name, seqs, is_t, depth, got):
    ebest, erp, ecols, calls = _reference(name, seqs, is_t, depth)
    best, row_ptr, cols, stats = got
    assert (np.diff(row_ptr) == np.diff(erp)).all(), "depth %d: rows differ in length from the reference loop" % depth
    assert len(cols) == len(ecols) and (cols == ecols).all(), "depth %d" % depth
    assert (best == ebest).all(), "depth %d" % depth
    assert stats["pairs_lanes"] >= calls
    return calls


@pytest.mark.parametrize("depth", DEPTHS)
def test_rows_and_counters_with_and_without_the_test(depth, monkeypatch):
    """Rows equal the reference loop with the test (ISOCON_DEBUG_VARIANT=nn2_block_filter) and without it (nn_no_block_filter, both
    names, no name); the listing is the same
    (pairs_lanes, rounds); at depths 5 and 17 pairs are rejected and exactly those are missing from the pair-per-lane launch.  (The
    `> 0` fails where the walk has no block test.)
    Checked on the CPU with the round scheme of tests/test_nn2set_depth_core.py (B doubling from 1 to 32 as in the driver) and the count of
    tests/qgram_ref.py (stride 2): of 818 / 3 968 / 9 228 listed pairs at depth 1 / 5 / 17, 0 / 1 714 / 5 431 have count > k (EXPECTED:
    the rejected set is exactly those, whatever the skip rule), all with distance -1 from the oracle; the set with N has 0 / 1 061 / 3 548."""
    seqs, is_t = _set(False)
    assert max(DEPTHS) < int(is_t.sum()) <= 50
    on = _graph(seqs, is_t, depth, monkeypatch, ON)
    off = _graph(seqs, is_t, depth, monkeypatch, "nn_no_block_filter")
    both = _graph(seqs, is_t, depth, monkeypatch, ON + ",nn_no_block_filter")          # "without the block filter" wins
    default = _graph(seqs, is_t, depth, monkeypatch)
    for got in (on, off, both, default):
        _assert_rows("clean", seqs, is_t, depth, got)
        for a, b in zip(got[:3], off[:3]):
            assert a.shape == b.shape and (a == b).all()
    for key in ("pairs_lanes", "scan_launches", "pairs_block_rejected", "pairs_lanes_aligned", "pairs_bytes", "full_pairs"):
        assert both[3][key] == off[3][key] and default[3][key] == off[3][key], key          # (the test is off unless asked for)
    s_on, s_off = on[3], off[3]
    print({key: (s_on[key], s_off[key]) for key in ("pairs_lanes", "scan_launches", "pairs_block_rejected", "pairs_lanes_aligned", "filter_kernel_ms", "kernel_ms")})
    assert s_on["pairs_lanes"] == s_off["pairs_lanes"] and s_on["scan_launches"] == s_off["scan_launches"]
    assert s_off["pairs_block_rejected"] == 0
    if depth >= 5:
        assert s_on["pairs_block_rejected"] > 0
        assert s_on["filter_kernel_ms"] > 0
    assert (s_on["pairs_lanes"], s_on["pairs_block_rejected"]) == EXPECTED[depth]
    assert s_on["pairs_lanes_aligned"] == s_off["pairs_lanes_aligned"] - s_on["pairs_block_rejected"]
    assert s_off["pairs_lanes_aligned"] == s_off["pairs_lanes"]
    assert s_on["pairs_bytes"] == 0 and s_off["pairs_bytes"] == 0


@pytest.mark.parametrize("depth", DEPTHS)
def test_nothing_to_probe(depth, monkeypatch):
    """sequences of 3 to 7 bases: no pair can be rejected, no task is made"""
    seqs, is_t = _short_set()
    assert depth < int(is_t.sum())
    got = _graph(seqs, is_t, depth, monkeypatch, ON)
    _assert_rows("short", seqs, is_t, depth, got)
    assert got[3]["pairs_block_rejected"] == 0
    assert got[3]["pairs_lanes_aligned"] == got[3]["pairs_lanes"]


@pytest.mark.parametrize("depth", DEPTHS)
def test_rows_with_n(depth, monkeypatch):
    """N in 2 % of the reads and 30 % of the candidates: their pairs are aligned on the bytes, never tested; the rest is tested as before"""
    seqs, is_t = _set(True)
    assert any("N" in s for s in seqs) and depth < int(is_t.sum())
    got = _graph(seqs, is_t, depth, monkeypatch, ON)
    _assert_rows("with_N", seqs, is_t, depth, got)
    assert got[3]["pairs_bytes"] > 0
    print("pairs_block_rejected", got[3]["pairs_block_rejected"])          # (anything from 0 up: the listing differs from the clean set's)
    assert got[3]["pairs_lanes_aligned"] == got[3]["pairs_lanes"] - got[3]["pairs_block_rejected"]
