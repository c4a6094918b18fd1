"""CPU: every designed case of tests/shw_cases.py sits where it claims -- its distance, its ends, its class, its round -- under the plain
restatement, the restatement agrees with the oracle's global distance on prefixes, and what the issue states about ends holds on a
random list.  No library load."""
import pytest

import shw_cases as C
from oracle import oracle as O


def lanes_of(group):
    for c in C.cases(group):
        assert len(c.targets) == len(c.ks) == len(c.lanes) > 0, c.name
        for i, (t, k, l) in enumerate(zip(c.targets, c.ks, c.lanes)):
            yield c, i, t, k, l, C.expected(group)[c.name, i]


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_every_claim_holds(group):
    seen = 0
    for c, i, t, k, l, (ed, ends) in lanes_of(group):
        P, n, h = len(c.query), len(t), l["h"]
        hu, endsu = C.restated_cached(c.query, t, None)
        assert h == hu and 0 <= h <= P and (ed, ends) == ((h, endsu) if k is None or h <= k else (-1, ())), (c.name, i)
        # where the ends of a hit lie, and how many there are at most
        assert all(P - h - 1 <= e <= min(n, P + h) - 1 for e in endsu) and 1 <= len(endsu) <= 2 * h + 1, (c.name, i)
        if "h_is" in l:
            assert h == l["h_is"], (c.name, i, h)
        if "ends" in l:
            assert list(ends) == l["ends"], (c.name, i, ends)
        if "has_end" in l:
            assert l["has_end"] in ends, (c.name, i, ends)
        if "hit" in l:
            assert (ed >= 0) == l["hit"] and (l["hit"] or k == h - 1), (c.name, i)
        if l.get("kernel") is False:
            assert not C.needs_kernel(P, n, C.clamp(k, P)) and ed == -1 and n - P == -k - 1, (c.name, i)
        if "same_as" in l:
            assert C.expected(group)[c.name, l["same_as"]] == (ed, ends), (c.name, i)
        if "in_round" in l:
            assert l["round"] == l["in_round"] and C.ROUND_THR[l["round"]] >= h and (l["round"] == 0 or C.ROUND_THR[l["round"] - 1] < h), (c.name, i)
        # the round and class the driver settles the pair in
        r, thr = C.settles(P, n, k, h)
        assert (r, None if thr is None else C.words(2 * thr + 1)) == (l["round"], l["words"]) and r is not None, (c.name, i)
        seen += 1
    assert seen >= 8


def test_group_a_covers_every_class_edge_at_and_below_the_threshold():
    hs, by_words, misses = set(), set(), 0
    for c, i, t, k, l, (ed, ends) in lanes_of("a"):
        assert l["h"] in C.CLASS_H and l["h"] == l["planted"], (c.name, i, l["h"], l["planted"])
        hs.add(l["h"])
        by_words.add(l["words"])
        misses += ed < 0
        if l["hit"]:
            assert k == l["h"] and l["words"] == C.words(2 * min(k, C.ROUND_THR[l["round"]]) + 1)
    assert hs == set(C.CLASS_H) and by_words == {1, 2, 4, 8} and misses >= 20
    assert [len(c.query) for c in C.cases("a")] == list(C.CLASS_P)
    big, = [c for c in C.cases("a") if len(c.query) == 300]
    assert {l["h"] for l in big.lanes} == set(C.CLASS_H)


def test_group_c_end_counts_and_columns():
    got = {c.name: [len(C.expected("c")[c.name, i][1]) for i in range(len(c.targets))] for c in C.cases("c")}
    assert got["c_a20"] == [11] and got["c_acgtc"] == [3] and got["c_a100_m64"] == [37, 37] and got["c_a70_m69"] == [2, 2]
    straddle = [c for c in C.cases("c") if c.name.startswith("c_straddle")]
    cols = {e + 1 for c in straddle for e in C.expected("c")[c.name, 0][1]}
    assert {32, 33, 64, 65} <= cols and len(straddle) == 11


def test_group_d_tiles_and_thresholds():
    for n in C.TILE_SIZES:
        c, = [c for c in C.cases("d") if c.name == "d_targets%d" % n]
        assert len(c.targets) == n and set(c.ks) == set(range(min(n, 32))) and len({len(t) for t in c.targets}) > min(n, 2) - 1
        assert all(l["round"] == 0 and l["words"] == 1 for l in c.lanes)
    multi = [c for c in C.cases("d") if c.name.startswith("d_multi")]
    assert len(multi) == 3 and all(c.targets[-1] == c.targets[2] for c in multi)


def test_group_e_rounds_and_the_far_pair():
    c, = C.cases("e")
    assert len(c.query) == 600 and set(c.ks) == {None}
    assert sorted({l["round"] for l in c.lanes}) == [0, 1, 2, 3] and [l["words"] for l in c.lanes] == [1, 1, 2, 2, 4, 4, 8, 8]
    hs = [l["h"] for l in c.lanes]
    assert 0 < hs[0] <= 31 == hs[1] < hs[2] <= 63 == hs[3] < hs[4] <= 127 == hs[5] < hs[6] <= 255 == hs[7]
    q, far = C.far_pair()
    h = C.restated(q, far, None)[0]
    assert h > 255 and C.settles(len(q), len(far), None, h) == (None, None)
    assert C.settles(len(q), len(far), 255, h) == (3, 255)          # under a threshold of 255 it is a plain miss


def test_restatement_equals_the_oracle_on_prefixes():
    seqs, q, t, k = C.random_list()
    for p in range(0, len(q), 40):
        x, y = seqs[q[p]], seqs[t[p]]
        h, ends = C.restated(x, y, None)
        d = [O.ed_dp(x, y[:j]) for j in range(1, len(y) + 1)]
        assert h == min(d) and ends == [j for j, v in enumerate(d) if v == h], p
    assert C.restated("", "ACG", None) == (-1, []) and C.restated("ACG", "", 5) == (-1, [])
    assert C.restated("ACGTC", "ACGTAC", 2) == (1, [3, 4, 5]) and C.restated("ACGTC", "ACGTAC", 0) == (-1, [])


def test_random_list_shape():
    seqs, q, t, k = C.random_list()
    assert len(q) == len(t) == len(k) == 2000 and all(1 <= len(s) <= 200 for s in seqs)
    hits = sum(C.restated_cached(seqs[a], seqs[b], kk)[0] >= 0 for a, b, kk in zip(q, t, k))
    assert 400 < hits < 1900 and None in k and 0 in k
