"""GPU: infix alignments beyond 512 diagonals (isocon_hw_pairs_wide = SeqStore.hw_pairs(wide=True): csrc/hw_full.hpp for the wide
pairs, the banded kernels for the others) against the oracle's full matrices -- all five outputs of every pair -- and through the
pipeline's functions (get_NN_graph_ignored_ends_edlib with ignore_ends_len = 150, edlib_traceback with k = 400)."""
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def hw_row(x, y, k):
    ed, start, end = O.hw_locate(x, y, k)
    if ed < 0:
        return [-1, -1, -1, 0, 0]
    _, ops = O.nw_path(x, y[start:end + 1])
    return [ed, start, end, ops[0][0] if ops[0][1] == "I" else 0, ops[-1][0] if ops[-1][1] == "I" else 0]


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, nmut):
    v = list(s)
    for _ in range(nmut):
        p = rng.randrange(len(v))
        r = rng.random()
        if r < 0.4:
            v[p] = rng.choice("ACGT")
        elif r < 0.7 and len(v) > 1:
            del v[p]
        else:
            v.insert(p, rng.choice("ACGT"))
    return "".join(v)


def is_wide(lq, lt, k):
    """The routing rule of isocon_hw_pairs_wide: a pair that needs a kernel and whose own band exceeds 512 diagonals."""
    return lq > 0 and lt > 0 and lt - lq >= -k and max(lt - lq, 0) + 2 * k + 1 > 512


def run(seqs, q, t, k, **kw):
    from isocon_amd.store import SeqStore
    st = SeqStore(seqs)
    try:
        return np.asarray(st.hw_pairs(q, t, k, **kw)).copy()
    finally:
        st.close()


def check_pairs(pairs, wide=True):
    """pairs = [(query, target, k)]: one call, every row against the oracle."""
    seqs, q, t, k = [], [], [], []
    for x, y, kk in pairs:
        q.append(len(seqs)); seqs.append(x)
        t.append(len(seqs)); seqs.append(y)
        k.append(kk)
    got = run(seqs, q, t, np.asarray(k, dtype=np.int32), wide=wide)
    exp = [hw_row(x, y, kk) for x, y, kk in pairs]
    for p, (g, e) in enumerate(zip(got.tolist(), exp)):
        assert g == e, (p, len(pairs[p][0]), len(pairs[p][1]), pairs[p][2])
    return got, exp


def embedded(rng, q, tlen, nmut=2):
    """A target of tlen bases that holds a copy of q with a few edits (cut to fit when the target is the shorter one)."""
    core = mutate(rng, q, nmut)[:tlen]
    a = rng.randint(0, tlen - len(core))
    return rnd(rng, a) + core + rnd(rng, tlen - a - len(core))


# ---- block edges -----------------------------------------------------------------------------------------------------------
def test_band_of_512_513_514_diagonals_at_every_block_edge():
    rng = random.Random(101)
    pairs, at512 = [], []
    for qlen in (1, 63, 64, 65, 128, 129, 640, 700):
        for band in (512, 513, 514):
            k = 100
            q = rnd(rng, qlen)
            if band == 512:
                at512.append(len(pairs))
            pairs.append((q, embedded(rng, q, qlen + band - 2 * k - 1), k))
    got, exp = check_pairs(pairs)
    assert sum(e[0] >= 0 for e in exp) >= 16
    narrow = [pairs[i] for i in at512]
    banded, _ = check_pairs(narrow, wide=False)                  # 512 diagonals: the banded kernels take them, the same rows
    assert banded.tolist() == got[at512].tolist()
    assert not any(is_wide(len(x), len(y), k) for x, y, k in narrow)
    assert all(is_wide(len(x), len(y), k) for i, (x, y, k) in enumerate(pairs) if i not in at512)


@pytest.mark.parametrize("k", [256, 300, 1000, 5000])
def test_large_thresholds(k):
    rng = random.Random(k)
    pairs = []
    for i in range(24):
        q = rnd(rng, rng.randint(300, 700))
        r = i % 4
        if r == 0:
            t = embedded(rng, q, rng.randint(300, 700), 5)
        elif r == 1:
            t = rnd(rng, rng.randint(300, 700))                                  # unrelated: a distance of about half the query
        elif r == 2:
            t = mutate(rng, q[rng.randint(0, 60):len(q) - rng.randint(0, 60)], 4)    # the query hangs over both ends
        else:
            t = rnd(rng, rng.randint(0, 50)) + mutate(rng, q, 8) + rnd(rng, rng.randint(0, 50))
        pairs.append((q, t, k))
    _, exp = check_pairs(pairs)
    assert sum(e[0] >= 0 for e in exp) >= 12 and sum(e[3] > 0 or e[4] > 0 for e in exp) >= 3


def test_the_pair_the_banded_entry_refuses():
    from isocon_amd.store import SeqStore
    x, y = "ACGTACGTAA", "ACGTACGTAAGG" * 30
    st = SeqStore([x, y])
    try:
        with pytest.raises(RuntimeError):
            st.hw_pairs([0], [1], [200])                # 350 + 400 + 1 diagonals > 512: isocon_hw_pairs itself stays as it is
        assert st.hw_pairs([0], [1], [200], wide=True).tolist() == [hw_row(x, y, 200)]
    finally:
        st.close()


@pytest.mark.parametrize("qlen", [4097, 4200])
def test_second_pass_of_the_block_loop(qlen):
    rng = random.Random(qlen)
    core = rnd(rng, qlen - 40)
    q = rnd(rng, 25) + core + rnd(rng, 15)
    pairs = [(q, mutate(rng, core, 6) + rnd(rng, 340 - 40), 600),          # target = query + 300, start 0: both passes of the trace store
             (q, rnd(rng, 260) + mutate(rng, core, 6) + rnd(rng, 80 - 40), 600),    # target = query + 300, inner start: the last column alone is kept
             (q, mutate(rng, core[:qlen - 340], 6), 600)]                  # target = query - 300, the query hangs over the end
    _, exp = check_pairs(pairs)
    assert all(e[0] >= 0 for e in exp) and exp[0][1] == 0 and exp[0][3] > 0 and exp[1][1] > 0


# ---- mixed list, launches cut by the trace budget --------------------------------------------------------------------------
def trace_bytes(m, ms):
    """csrc/hw_full_core.hpp hwf_trace_units, restated: the store of a query of m rows over ms columns."""
    r32 = lambda u: (u + 31) // 32 * 32
    blocks = (m + 63) // 64
    passes = (blocks + 63) // 64
    last = blocks - 64 * (passes - 1)
    return 16 * (r32((blocks + 1) // 2) + (passes - 1) * r32((ms + 63) * 64) + r32((ms + last - 1) * last))


def test_mixed_list_and_one_launch_per_wide_pair(monkeypatch):
    rng = random.Random(77)
    seqs, q, t, k = [], [], [], []
    for i in range(300):
        core = rnd(rng, rng.randint(300, 330))
        x = rnd(rng, rng.choice([0, 0, 3])) + mutate(rng, core, rng.choice([0, 2, 6])) + rnd(rng, rng.choice([0, 0, 4]))
        if i % 2:
            y = rnd(rng, rng.randint(250, 300)) + core + rnd(rng, rng.randint(230, 260))         # 480+ longer, k = 20: wide
        else:
            y = rnd(rng, rng.randint(0, 40)) + core + rnd(rng, rng.randint(0, 40))               # narrow
        if i % 25 == 0:
            y = rnd(rng, len(y))                                                                 # no hit
        q.append(len(seqs)); seqs.append(x)
        t.append(len(seqs)); seqs.append(y)
        k.append(20)
    order = list(range(300))
    rng.shuffle(order)
    q = np.asarray(q, dtype=np.uint32)[order]; t = np.asarray(t, dtype=np.uint32)[order]; k = np.asarray(k, dtype=np.int32)[order]
    wide = np.asarray([is_wide(len(seqs[a]), len(seqs[b]), int(kk)) for a, b, kk in zip(q, t, k)])
    assert 120 <= wide.sum() <= 180
    got = run(seqs, q, t, k, wide=True)
    assert got[~wide].tolist() == run(seqs, q[~wide], t[~wide], k[~wide]).tolist()
    exp = np.asarray([hw_row(seqs[a], seqs[b], int(kk)) for a, b, kk in zip(q, t, k)])
    assert got[wide].tolist() == exp[wide].tolist()
    assert (exp[wide][:, 0] >= 0).sum() >= 100 and (exp[wide][:, 0] < 0).sum() >= 3
    # a budget that holds the largest store of the call and not two of the smallest: every wide hit is a launch of its own
    need = [trace_bytes(len(seqs[a]), int(e[2]) + 1) for a, e, w in zip(q, exp, wide) if w and e[0] >= 0]
    assert max(need) < 2 * min(need)
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "hw_trace_budget=%d" % max(need))
    again = run(seqs, q, t, k, wide=True)
    assert again.tolist() == got.tolist()
    # and one byte less: the largest pair is refused, with its sizes
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "hw_trace_budget=%d" % (max(need) - 1))
    with pytest.raises(RuntimeError, match="unsupported request.*needs %d bytes" % max(need)):
        run(seqs, q, t, k, wide=True)


# ---- insertion runs ---------------------------------------------------------------------------------------------------------
def insertion_run_pairs(seed=5):
    rng = random.Random(seed)
    pairs = []
    for a in (0, 1, 5, 40):
        for b in (0, 1, 5, 40):
            for fl in (0, 3, 60):
                for fr in (0, 3, 60):
                    core = rnd(rng, rng.randint(100, 140))
                    pairs.append((rnd(rng, a) + core + rnd(rng, b), rnd(rng, fl) + core + rnd(rng, fr), 260))
    return pairs


def test_insertion_runs_are_exercised():
    pairs = insertion_run_pairs()
    exp = [hw_row(x, y, kk) for x, y, kk in pairs]
    assert sum(e[3] > 0 for e in exp) >= 20 and sum(e[4] > 0 for e in exp) >= 20 and sum(e[0] >= 0 and e[3] == 0 and e[4] == 0 for e in exp) >= 20
    assert all(is_wide(len(x), len(y), kk) for x, y, kk in pairs)
    check_pairs(pairs)


# ---- negatives ----------------------------------------------------------------------------------------------------------------
def test_negatives_and_errors():
    from isocon_amd.store import SeqStore
    rng = random.Random(9)
    a, b = rnd(rng, 400), rnd(rng, 700)
    seqs = [a, b, a[:50], "", mutate(rng, a, 3) + rnd(rng, 300)]
    st = SeqStore(seqs)
    try:
        none = [-1, -1, -1, 0, 0]
        r = st.hw_pairs([0, 0, 2, 3, 0, 0], [1, 2, 3, 1, 3, 4], [120, 300, 300, 300, 300, 300], wide=True)
        assert r[0].tolist() == none and hw_row(a, b, 120) == none              # distance above k (wide: 300 + 241 diagonals)
        assert r[1].tolist() == none                                            # query longer than target + k
        banded = st.hw_pairs([2, 3, 0], [3, 1, 3], [5, 5, 5])                    # an empty sequence: what the banded entry gives
        assert r[2:5].tolist() == banded.tolist() == [none] * 3
        assert r[5].tolist() == hw_row(a, seqs[4], 300)
        with pytest.raises(RuntimeError, match="bad argument"):
            st.hw_pairs([0], [1], [-1], wide=True)
        with pytest.raises(RuntimeError, match="unsupported request"):
            st.hw_pairs([0], [1], [2 ** 20 + 1], wide=True)
        with pytest.raises(RuntimeError, match="bad argument"):
            st.hw_pairs([0], [len(seqs)], [300], wide=True)
        assert st.hw_pairs([0], [4], [300], wide=True).tolist() == [hw_row(a, seqs[4], 300)]          # usable afterwards
        assert st.hw_pairs([0], [1], [2 ** 20], wide=True)[0][0] == hw_row(a, b, 2 ** 20)[0]
    finally:
        st.close()
    st5 = SeqStore([a, b + "N"])                                   # five symbols: the planes cannot hold the set
    try:
        with pytest.raises(RuntimeError, match="symbol outside ACGT"):
            st5.hw_pairs([0], [1], [300], wide=True)
    finally:
        st5.close()


# ---- through the pipeline's functions -------------------------------------------------------------------------------------------
def candidate_families(seed=2024):
    """~60 candidates of 240 - 500 bases in 3 families: one transcript per family, members = a window of it that always holds the
    same 240 inner bases (end extensions of 0 - 130 bases on either side) with at most 4 internal edits each."""
    rng = random.Random(seed)
    cands = {}
    for fam in range(3):
        full = rnd(rng, 130 + 240 + 130)
        for i in range(20):
            a, b = rng.choice([0, 5, 40, 100, 130]), rng.choice([0, 5, 40, 100, 130])
            inner = mutate(rng, full[130:370], rng.randint(0, 4))
            cands["f%d_%d" % (fam, i)] = full[130 - a:130] + inner + full[370:370 + b]
    return cands


class Params(object):
    nr_cores = 1
    neighbor_search_depth = 2 ** 32
    verbose = False

    def __init__(self, ignore_ends_len):
        self.ignore_ends_len = ignore_ends_len


@pytest.fixture
def spy(monkeypatch):
    from isocon_amd import end_invariant_functions as END
    calls = []
    real = END.SeqStore.hw_pairs

    def hw_pairs(self, q, t, k, **kw):
        calls.append((np.asarray(self.lens)[np.asarray(q, dtype=np.int64)], np.asarray(self.lens)[np.asarray(t, dtype=np.int64)], np.asarray(k), dict(kw)))
        return real(self, q, t, k, **kw)
    monkeypatch.setattr(END.SeqStore, "hw_pairs", hw_pairs)
    return calls


def test_candidate_graph_with_ignore_ends_len_150(spy):
    from isocon_amd import end_invariant_functions as END
    cands = candidate_families()
    exp = O.get_NN_graph_ignored_ends_edlib(dict(cands), Params(150))
    assert sum(len(v) for v in exp.values()) >= 30
    got = END.get_NN_graph_ignored_ends_edlib(dict(cands), Params(150))
    assert {a: dict(nb) for a, nb in got.items()} == {a: dict(nb) for a, nb in exp.items()}
    assert len(spy) == 1 and spy[0][3].get("wide") is True
    lq, lt, k, _ = spy[0]
    nwide = sum(is_wide(int(a), int(b), int(kk)) for a, b, kk in zip(lq, lt, np.broadcast_to(k, lq.shape)))
    assert 0 < nwide < len(lq)                                  # both kinds of pairs in the one call


def test_candidate_graph_default_takes_the_banded_path(spy):
    from isocon_amd import end_invariant_functions as END
    cands = candidate_families()
    got = END.get_NN_graph_ignored_ends_edlib(dict(cands), Params(15))
    exp = O.get_NN_graph_ignored_ends_edlib(dict(cands), Params(15))
    assert {a: dict(nb) for a, nb in got.items()} == {a: dict(nb) for a, nb in exp.items()}
    assert len(spy) == 1 and not spy[0][3].get("wide", False)


def test_traceback_with_k_400(spy):
    from isocon_amd import end_invariant_functions as END
    rng = random.Random(31)
    full = rnd(rng, 900)
    for x, y in [(full[100:500], full), (rnd(rng, 60) + full[300:700] + rnd(rng, 200), full), (full[:350], mutate(rng, full[:700], 9)), (rnd(rng, 300), rnd(rng, 500))]:
        assert END.edlib_traceback(x, y, mode="HW", task="path", k=400, end_threshold=150) == O.edlib_traceback_hw(x, y, k=400, end_threshold=150)
    assert len(spy) == 4 and all(c[3].get("wide") is True for c in spy)
    assert END.edlib_traceback(full[100:500], full[50:600], mode="HW", task="path", k=100, end_threshold=15) == O.edlib_traceback_hw(full[100:500], full[50:600], k=100, end_threshold=15)
    assert not spy[4][3].get("wide", False)                      # 150 + 201 diagonals: the call it has always been
