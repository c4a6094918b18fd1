"""GPU: the banded route of the alignment paths (csrc/nw_band.hpp behind isocon_ed_path_pairs / isocon_hw_path_pairs): hits whose corridor
fits 256 diagonals are traced one pair per lane through a sliding window.  Results against the oracle (oracle.nw_path / oracle.hw_path)
and against the un-banded route (ISOCON_DEBUG_VARIANT=nwp_unbanded), the classes and the trace volume through store.path_last_stats(),
the band budget, and a pair the un-banded store cannot hold."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from test_nw_band_core import (NOT_BANDED, band_class, banded_path_cases, edge_cases, expect, expect_window, sweep_cases, tie_cases,
                               window_cases)
from test_nw_path_core import mutate, rnd

pytestmark = pytest.mark.gpu


def store_of(pairs):
    from isocon_amd.store import SeqStore
    seqs = sorted({s for p in pairs for s in p})
    index = {s: i for i, s in enumerate(seqs)}
    return SeqStore(seqs), [index[q] for q, _ in pairs], [index[t] for _, t in pairs]


def decoded(ops, ops_ptr, p):
    return [(int(o) >> 4, "=XID"[int(o) & 15]) for o in ops[int(ops_ptr[p]):int(ops_ptr[p + 1])]]


def stats():
    from isocon_amd.store import path_last_stats
    return path_last_stats()


def class_counts(pairs):
    """hits per class as the CPU test derives them from the oracle's distance and the lengths: {1: .., 2: .., 4: .., NOT_BANDED: ..}"""
    out = {1: 0, 2: 0, 4: 0, NOT_BANDED: 0}
    for q, t in pairs:
        out[band_class(len(q), len(t), expect(q, t)[0])] += 1
    return out


def check_stats(s, counts):
    assert (s["hits_w1"], s["hits_w2"], s["hits_w4"], s["hits_unbanded"]) == (counts[1], counts[2], counts[4], counts[NOT_BANDED])
    assert s["hits"] == sum(counts.values())
    assert (s["launches_unbanded"] > 0) == (counts[NOT_BANDED] > 0) and (s["trace_bytes_unbanded"] > 0) == (counts[NOT_BANDED] > 0)
    assert s["launches_band"] >= sum(1 for w in (1, 2, 4) if counts[w]) and s["trace_bytes_band"] > 0


@pytest.fixture(scope="module")
def case_list():
    """the lists (a) - (c) of the CPU test in one store"""
    edges = [(q, t) for _, q, t in edge_cases()]
    pairs = banded_path_cases() + tie_cases() + sweep_cases() + edges
    st, a, b = store_of(pairs)
    yield pairs, st, a, b, len(pairs) - len(edges)
    st.close()


@pytest.mark.parametrize("kmode", ["none", "ed", "ed+1"])
def test_lists_against_oracle(case_list, kmode, monkeypatch):
    pairs, st, a, b, first_edge = case_list
    d = np.array([expect(q, t)[0] for q, t in pairs])
    k = {"none": None, "ed": d, "ed+1": d + 1}[kmode]
    ed, ops, ops_ptr = st.ed_path_pairs(a, b, k)
    s = stats()
    assert ed.tolist() == d.tolist() and int(ops_ptr[-1]) == len(ops)
    for p, (q, t) in enumerate(pairs):
        assert decoded(ops, ops_ptr, p) == expect(q, t)[1], (q, t)
    counts = class_counts(pairs)
    assert counts[1] > 100 and counts[2] >= 12 and counts[4] >= 12
    check_stats(s, counts)
    # no hit is un-banded except the blocks of 256 bases
    not_banded = [p for p, (q, t) in enumerate(pairs) if band_class(len(q), len(t), int(d[p])) == NOT_BANDED]
    assert len(not_banded) == 6 and all(p >= first_edge and int(d[p]) == 256 for p in not_banded)
    # ... and the same arrays as the un-banded route gives
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_unbanded")
    again = st.ed_path_pairs(a, b, k)
    s = stats()
    assert [x.tolist() for x in again] == [ed.tolist(), ops.tolist(), ops_ptr.tolist()]
    assert s["hits_unbanded"] == s["hits"] == len(pairs) and s["hits_w1"] + s["hits_w2"] + s["hits_w4"] == 0 and s["launches_band"] == 0


def mixed_list():
    """130 pairs with lengths 1 .. 300, classes mixed: a few edits (class 1), a block of 70 or of 130 bases deleted (classes 2 and 4),
    unrelated sequences (any class): two full waves and a partly filled one in class 1, lanes that finish at different columns"""
    rng = random.Random(130)
    pairs = []
    for p in range(130):
        n = 1 + (p * 23) % 300
        q = rnd(rng, n)
        if p % 10 == 3 and n > 150:
            t = q[:40] + q[110:]
        elif p % 10 == 7 and n > 200:
            t = q[:30] + q[160:]
        elif p % 10 == 9:
            t = rnd(rng, rng.randint(1, 300))
        else:
            t = mutate(rng, q, rng.randint(0, 6))
        pairs.append((q, t) if p % 2 else (t, q))
    return [(q, t) for q, t in pairs if q and t]


def test_mixed_classes_and_partly_filled_waves():
    pairs = mixed_list()
    assert len(pairs) == 130 and {len(q) for q, _ in pairs} | {len(t) for _, t in pairs} >= {1, 300}
    st, a, b = store_of(pairs)
    ed, ops, ops_ptr = st.ed_path_pairs(a, b)
    s = stats()
    for p, (q, t) in enumerate(pairs):
        assert (int(ed[p]), decoded(ops, ops_ptr, p)) == expect(q, t), (q, t)
    counts = class_counts(pairs)
    assert counts[1] > 64 and counts[1] % 64 != 0 and counts[2] >= 3 and counts[4] >= 3
    check_stats(s, counts)
    st.close()


def test_window_form_against_oracle():
    pairs = window_cases()
    st, a, b = store_of(pairs)
    rows, ops, ops_ptr = st.hw_path_pairs(a, b)
    s = stats()
    counts = {1: 0, 2: 0, 4: 0, NOT_BANDED: 0}
    for p, (q, t) in enumerate(pairs):
        e_ed, start, cols, e_ops = expect_window(q, t)
        assert rows[p, :3].tolist() == [e_ed, start, start + cols - 1], (q, t)
        assert decoded(ops, ops_ptr, p) == e_ops, (q, t)
        counts[band_class(len(q), cols, e_ed)] += 1
    # every class in one call, and three blocks beyond the band scattered among them: band hits behind an un-banded prefix on the device
    assert counts[1] >= 10 and counts[2] >= 6 and counts[4] >= 6 and counts[NOT_BANDED] == 3
    check_stats(s, counts)
    # a call without pairs describes itself, not the call before it
    st.hw_path_pairs([], [])
    assert stats()["hits"] == 0 and stats()["trace_bytes_band"] == 0 and stats()["launches_band"] == 0
    st.close()


def test_band_budget(monkeypatch):
    rng = random.Random(13)
    pairs = []
    for _ in range(9):
        q = rnd(rng, rng.randint(180, 220))
        pairs.append((q, mutate(rng, q, 4)))
    st, a, b = store_of(pairs)
    want = st.ed_path_pairs(a, b)
    s0 = stats()
    for p, (q, t) in enumerate(pairs):
        assert (int(want[0][p]), decoded(want[1], want[2], p)) == expect(q, t)
    cols32 = [(len(t) + 31) // 32 * 32 for _, t in pairs]          # a lane's columns, in the kernel's blocks of 32
    region = max(cols32) * 9 * 16                                   # the one wave of the list: [column][word][lane] x 16 bytes, 9 lanes
    assert (s0["hits_w1"], s0["launches_band"], s0["trace_bytes_band"]) == (9, 1, region)
    # the budget of exactly that region: still one launch
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_band_budget=%d" % region)
    again = st.ed_path_pairs(a, b)
    assert [x.tolist() for x in again] == [x.tolist() for x in want] and stats()["launches_band"] == 1
    # room for three of the longest lanes: the wave is cut into waves of at most three lanes, each a launch of its own
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_band_budget=%d" % (3 * max(cols32) * 16))
    again = st.ed_path_pairs(a, b)
    s = stats()
    assert [x.tolist() for x in again] == [x.tolist() for x in want]
    assert s["launches_band"] >= 3 and s["hits_w1"] == 9 and s["hits_unbanded"] == 0 and s["trace_bytes_band"] <= region
    # one byte less than the longest pair needs on its own: refused, with its sizes
    need = max(cols32) * 16
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_band_budget=%d" % (need - 1))
    with pytest.raises(RuntimeError, match=r"unsupported request.*a query of \d+ bases against a target of \d+ bases needs %d bytes" % need):
        st.ed_path_pairs(a, b)
    st.close()


def test_trace_bytes_of_class_one():
    rng = random.Random(128)
    n = 100
    pairs = []
    for _ in range(128):
        q = rnd(rng, n)
        v = list(q)
        for _ in range(3):
            v[rng.randrange(n)] = rng.choice("ACGT")
        pairs.append((q, "".join(v)))
    st, a, b = store_of(pairs)
    ed, ops, ops_ptr = st.ed_path_pairs(a, b)
    s = stats()
    for p, (q, t) in enumerate(pairs):
        assert (int(ed[p]), decoded(ops, ops_ptr, p)) == expect(q, t)
    assert s["hits_w1"] == 128 and s["hits_unbanded"] == 0
    assert 0 < s["trace_bytes_band"] <= 2 * 64 * 16 * (n + 64)
    st.close()


def planted_pair(n, edits, seed):
    """two sequences of about n bases that differ by `edits` planted edits, far apart"""
    rng = random.Random(seed)
    q = "".join(rng.choice("ACGT") for _ in range(n))
    v = list(q)
    for e in range(edits, 0, -1):          # from the back, so that the positions stay those of q
        p = e * (n // (edits + 1))
        kind = e % 3
        if kind == 0:
            v[p] = "ACGT"[("ACGT".index(v[p]) + 1) % 4]
        elif kind == 1:
            del v[p]
        else:
            v.insert(p, rng.choice("ACGT"))
    return q, "".join(v)


def test_pair_beyond_the_unbanded_store(monkeypatch):
    """two 66 000-base sequences 20 edits apart: the un-banded store of the pair would be about 1.09 GB, above the 1 GiB budget"""
    from isocon_amd.store import SeqStore
    q, t = planted_pair(66000, 20, 66)
    assert len(q) * len(t) > 2 ** 32
    st = SeqStore([q, t])
    want = int(st.ed_pairs([0], [1])[0])
    assert 0 < want <= 20
    ed, ops, ops_ptr = st.ed_path_pairs([0], [1], 64)
    s = stats()
    assert int(ed[0]) == want
    assert (s["hits_w1"], s["hits_unbanded"], s["launches_band"]) == (1, 0, 1) and s["trace_bytes_band"] <= 16 * (len(t) + 32)
    # the ops turn the query into the target; '=' columns are equal, 'X' columns differ
    i = j = 0
    n = {c: 0 for c in "=XID"}
    qa, ta = np.frombuffer(q.encode(), dtype=np.uint8), np.frombuffer(t.encode(), dtype=np.uint8)
    path = decoded(ops, ops_ptr, 0)
    for length, c in path:
        n[c] += length
        if c == "=":
            assert np.array_equal(qa[i:i + length], ta[j:j + length])
        elif c == "X":
            assert len(qa[i:i + length]) == length == len(ta[j:j + length]) and not (qa[i:i + length] == ta[j:j + length]).any()
        i += length if c != "D" else 0
        j += length if c != "I" else 0
    assert (i, j) == (len(q), len(t)) and n["X"] + n["I"] + n["D"] == want
    assert all(x[1] != y[1] for x, y in zip(path, path[1:])) and all(length > 0 for length, _ in path)
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "nwp_unbanded")
    with pytest.raises(RuntimeError, match="unsupported request.*needs \\d+ bytes"):
        st.ed_path_pairs([0], [1], 64)
    st.close()
