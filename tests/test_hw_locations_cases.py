"""CPU: the designed inputs of isocon_hw_locations (tests/hw_locations_cases.py) have the properties they were built for -- every claim
of every lane under the plain restatement --, the restatement is tied to the oracle on every designed pair (first location =
oracle.hw_locate, every location has distance h and no smaller start inside the reach of h has), coverage totals per group, and the
random list of the GPU consistency test is cheap enough for the restatement."""
import time

import pytest

import hw_locations_cases as C
from oracle import oracle as O


def check_lane(c, i, got):
    q, t, k, claim = c.query, c.targets[i], c.ks[i], c.lanes[i]
    h, locs = got
    where = (c.name, i, claim, h, locs[:4])
    P, delta = len(q), len(t) - len(q)
    # ---- the oracle ties ----
    oh, os_, oe = O.hw_locate(q, t, k)
    assert oh == h, where
    if h < 0:
        assert not locs and O.hw_locate(q, t, -1)[0] == claim["dist"] > k, where
        return
    assert locs and locs[0] == (os_, oe), where
    assert [e for s, e in locs] == sorted({e for s, e in locs}), where
    for s, e in locs:
        assert 0 <= s <= e < len(t) and O.ed_dp(q, t[s:e + 1]) == h, where + ((s, e),)
    # no smaller start inside the reach of h (every location of the small cases, the first and the last of the long ones)
    for s, e in (locs if P <= 130 else [locs[0], locs[-1]]):
        assert all(O.ed_dp(q, t[s2:e + 1]) > h for s2 in range(max(0, e + 1 - P - h), s)), where + ((s, e),)
    # ---- the claims ----
    assert claim["dist"] == h <= k, where
    if "first" in claim:
        assert locs[0] == tuple(claim["first"]), where
    if "locs" in claim:
        assert list(locs) == [tuple(x) for x in claim["locs"]], where
    if "ends" in claim:
        assert [e for s, e in locs] == list(claim["ends"]), where
    if "n_ends" in claim:
        assert len(locs) == claim["n_ends"], where
    if "ends_w" in claim:
        assert C.words(C.rows(delta, h)) == claim["ends_w"], where
    if "starts_w" in claim:
        assert C.words(2 * h + 1) == claim["starts_w"], where
    if "locate_w" in claim:
        assert C.words(C.rows(delta, k)) == claim["locate_w"] > C.words(C.rows(delta, h)), where
    if claim.get("gap_above"):
        last = C._last_row(q, t, True)[1:]
        for (s0, e0), (s1, e1) in zip(locs, locs[1:]):
            assert e1 - e0 > 64 and last[e0 + 1:e1].min() > h and last[e0 + 33:e1 - 33].min() > k, where


@pytest.mark.parametrize("group", C.ALL_GROUPS)
def test_every_claim_holds(group):
    exp = C.expected(group)
    names = [c.name for c in C.cases(group)]
    assert len(set(names)) == len(names) > 0
    for c in C.cases(group):
        assert c.group == group and len(c.targets) == len(c.ks) == len(c.lanes) > 0 and c.what
        assert all(set(s) <= set("ACGT") and s for s in [c.query] + c.targets)
        assert all(len(t) - len(c.query) < -k or C.words(C.rows(len(t) - len(c.query), k)) for t, k in zip(c.targets, c.ks))          # within the banded limit
        for i in range(len(c.targets)):
            check_lane(c, i, exp[c.name, i])


def hits_of(group):
    exp = C.expected(group)
    return [(c, i, exp[c.name, i]) for c in C.cases(group) for i in range(len(c.targets)) if exp[c.name, i][0] >= 0]


def test_coverage_bands():
    hits = hits_of("a")
    assert {C.rows(len(c.targets[i]) - len(c.query), h) for c, i, (h, locs) in hits} >= set(C.ENDS_EDGES)
    assert {h for c, i, (h, locs) in hits} >= set(C.START_EDGES)
    assert {C.words(C.rows(len(c.targets[i]) - len(c.query), h)) for c, i, (h, locs) in hits} == {1, 2, 4, 8}
    assert {C.words(2 * h + 1) for c, i, (h, locs) in hits} == {1, 2, 4, 8}
    wide = [(c, i) for c, i, r in hits if "locate_w" in c.lanes[i]]
    assert {(c.lanes[i]["locate_w"], c.lanes[i]["ends_w"]) for c, i in wide} >= {(4, 1), (8, 2), (8, 4)}
    assert any(r[0] < 0 for r in C.expected("a").values())


def test_coverage_columns_and_degenerate():
    hits = hits_of("b")
    ends = {e for c, i, (h, locs) in hits for s, e in locs}
    assert ends >= set(C.BLOCK_ENDS)
    assert any(e + 1 == len(c.query) - h for c, i, (h, locs) in hits for s, e in locs if h > 0)                # the first eligible column
    assert any(locs[-1][1] == len(c.targets[i]) - 1 for c, i, (h, locs) in hits)                               # the last column
    assert any(len(locs) == 2 and locs[0][1] // 32 == locs[1][1] // 32 for c, i, (h, locs) in hits)           # two ends in one block
    assert sum(bool(c.lanes[i].get("gap_above")) for c, i, r in hits) == 12
    assert {len(locs) for c, i, (h, locs) in hits if c.name.startswith("b_run")} == {2, 3, 6}
    assert all(all(b[1] == a[1] + 1 for a, b in zip(locs, locs[1:])) for c, i, (h, locs) in hits if c.name.startswith("b_run"))
    exp = C.expected("c")
    assert [len(exp["c_exact_x%d" % r, 0][1]) for r in C.COPIES] == list(C.COPIES)
    assert exp["c_h_eq_k", 0][0] == 2 and exp["c_h_eq_k", 1] == (-1, ())
    assert all(len(exp[c.name, 0][1]) == len(c.targets[0]) and exp[c.name, 0][0] == len(c.query) for c in C.cases("c") if c.name.startswith("c_all"))
    assert any(len(c.query) == 1 for c in C.cases("c")) and any(len(t) == 1 for c in C.cases("c") for t in c.targets)
    assert any(len(t) - len(c.query) == -k and exp[c.name, i][0] == k > 0 for c in C.cases("c") for i, (t, k) in enumerate(zip(c.targets, c.ks)))
    assert any(len(t) - len(c.query) < -k for c in C.cases("c") for t, k in zip(c.targets, c.ks))


def test_coverage_tiles():
    assert sorted(len(c.targets) for c in C.cases("d") if c.name.startswith("d_targets")) == sorted(C.TILE_SIZES)
    for c in C.cases("d"):
        if c.name.startswith("d_targets") and len(c.targets) >= 63:
            tiles = C.ends_tiles(c, "d")
            assert len(tiles) == (len(c.targets) + 63) // 64 and all(w == 1 for w, lanes in tiles)
    c, = [c for c in C.cases("d") if c.name == "d_1_and_40"]
    exp = C.expected("d")
    assert [len(exp[c.name, i][1]) for i in range(3)] == [40, 1, 30]
    assert C.ends_tiles(c, "d") == [(8, [0, 1, 2])]
    c, = C.cases("e")
    exp = C.expected("e")
    own = [C.rows(len(t) - len(c.query), exp[c.name, i][0]) for i, t in enumerate(c.targets)]
    assert all(C.words(r) == 8 for r in own) and [w for w, lanes in C.ends_tiles(c, "e")] == [8, 8]
    assert C.rows(max(len(t) - len(c.query) for t in c.targets), max(exp[c.name, i][0] for i in range(2))) > 512
    assert C.rows(max(len(t) - len(c.query) for t in c.targets), max(c.ks)) > 512 >= max(C.rows(len(t) - len(c.query), k) for t, k in zip(c.targets, c.ks))


def test_random_list_is_cheap_and_rich():
    seqs, q, t, k = C.random_list()
    assert len(q) == 300 and all(20 <= len(seqs[i]) <= 200 for i in q)
    assert all(len(seqs[a]) - kk <= len(seqs[b]) <= len(seqs[a]) + 150 or len(seqs[b]) == 1 for a, b, kk in zip(q, t, k))
    t0 = time.time()
    res = [C.restated_cached(seqs[a], seqs[b], kk) for a, b, kk in zip(q, t, k)]
    assert time.time() - t0 < 20
    hits = [r for r in res if r[0] >= 0]
    assert len(hits) >= 100 and sum(len(r[1]) >= 2 for r in hits) >= 40 and sum(r[0] < 0 for r in res) >= 40
    assert all(C.words(C.rows(len(seqs[b]) - len(seqs[a]), kk)) for a, b, kk in zip(q, t, k))
    for (a, b, kk), (h, locs) in zip(zip(q, t, k), res):
        assert O.hw_locate(seqs[a], seqs[b], kk) == ((h,) + locs[0] if h >= 0 else (-1, -1, -1))
