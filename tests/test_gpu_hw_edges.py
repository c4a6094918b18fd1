"""GPU: the banded infix kernels (isocon_hw_pairs: csrc/hw.hpp, hw_core.hpp, hw_tiles.hpp, hw_host.inc) on the designed inputs of
tests/hw_edge_cases.py -- every class and segment edge, multi-lane tiles, promotion, more tiles than the finish grid -- against the oracle's
full matrices: all five values of EVERY designed pair, through the host-built tiles and through the device-built tiles, with the route,
the classes and the grid of the call read from store.hw_last_stats().  tests/test_hw_edge_cases.py shows on the CPU that the inputs sit
where they claim to."""
import random

import numpy as np
import pytest

import hw_edge_cases as E

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 4, 8)
BYSTANDER = "".join(random.Random(900).choice("ACGT") for _ in range(900))


def hw_call(monkeypatch, seqs, q, t, k, route, method="hw_pairs", **kw):
    """One call on a store of `seqs`: (rows of the pairs, hw_last_stats()).  route "host": tiles built on the host; "device": the pairs
    repeated in a shuffled order until there are 2048, the tiles built on the device, all replicas of a pair required to be equal."""
    from isocon_amd.store import SeqStore, hw_last_stats
    q, t, k = np.asarray(q, dtype=np.uint32), np.asarray(t, dtype=np.uint32), np.asarray(k, dtype=np.int32)
    n = len(q)
    if route == "host":
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "hw_host_tiles=1")
        order = np.arange(n)
    else:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
        order = np.tile(np.arange(n), (2048 + n - 1) // n)
        random.Random(n).shuffle(order)
        assert len(order) >= 2048
    st = SeqStore(seqs)
    try:
        got = getattr(st, method)(q[order], t[order], k[order], **kw)
        got = np.asarray(got[0] if method == "hw_path_pairs" else got).copy()
        stats = hw_last_stats()
    finally:
        st.close()
    first = np.full(n, -1, dtype=np.int64)
    first[order[::-1]] = np.arange(len(order))[::-1]
    assert (got == got[first][order]).all(), "replicas of a pair differ"
    return got[first].tolist(), stats, len(order)


def expected(owner, group_of):
    return [E.oracle_rows(group_of[c.name])[c.name, lane] for c, lane in owner]


def compare(got, exp, owner):
    bad = [(c.name, lane, g, e) for g, e, (c, lane) in zip(got, exp, owner) if g != e]
    assert not bad, (len(bad), len(got), bad[:5])


def group_of_cases(groups):
    return {c.name: g for g in groups for c in E.cases(g)}


def own_classes(owner, exp):
    """classes of the LOCATE bands of the pairs that need a kernel, and of the START / TRACE bands of the hits"""
    loc = {E.words(E.rows(len(c.targets[i]) - len(c.query), c.ks[i])) for c, i in owner if len(c.targets[i]) - len(c.query) >= -c.ks[i]}
    fin = {E.words(2 * c.ks[i] + 1) for (c, i), e in zip(owner, exp) if e[0] >= 0}
    return loc, fin


def check_counts(stats, route, n_sent, owner, exp):
    reps = n_sent // len(owner)
    assert stats["route"] == (0 if route == "host" else 1) and stats["retried_host"] == 0 and stats["pairs"] == n_sent
    need = sum(len(c.targets[i]) - len(c.query) >= -c.ks[i] for c, i in owner)
    assert stats["need_kernel"] == need * reps and stats["hits"] == sum(e[0] >= 0 for e in exp) * reps


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("group", [g for g in E.ALL_GROUPS if g != "i"])
def test_group_equals_oracle(monkeypatch, group, route):
    seqs, q, t, k, owner = E.flatten(E.cases(group), bystander=BYSTANDER if group == "d" else None)
    exp = expected(owner, group_of_cases([group]))
    got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, route)
    compare(got, exp, owner)
    check_counts(stats, route, n_sent, owner, exp)
    loc = {w for w in CLASSES if stats["locate_tiles_w%d" % w]}
    fin = {w for w in CLASSES if stats["finish_tiles_w%d" % w]}
    if group in "abg":
        # a pair list of these groups repeats (query, delta, k) or varies delta by a base or two inside a class: the tiles' classes are the pairs' own
        assert (loc, fin) == own_classes(owner, exp) and loc == fin == set(CLASSES)
    if group[0] == "j":
        W = int(group[1])
        assert E.finish_grid_cap(W) == (4096, 2304)[W - 1]
        assert fin == {W} and stats["finish_tiles_w%d" % W] == len(owner) * (n_sent // len(owner)) == E.finish_grid_cap(W) + 200
        assert stats["finish_grid_w%d" % W] == E.finish_grid_cap(W) < stats["finish_tiles_w%d" % W]          # some workgroup ran two tiles on one store
    for w in CLASSES:
        assert (stats["finish_grid_w%d" % w] > 0) == (stats["finish_tiles_w%d" % w] > 0) and stats["finish_grid_w%d" % w] <= stats["finish_tiles_w%d" % w]


@pytest.mark.parametrize("m", E.BLOCK_TARGET_LENGTHS)
def test_designed_target_is_the_longest_of_its_store(monkeypatch, m):
    """the words behind the last chunk of the planes read as zeros: nothing of another sequence follows the designed targets"""
    case, = [c for c in E.cases("d") if c.name == "d_m%d" % m]
    seqs, q, t, k, owner = E.flatten([case])
    assert max(len(s) for s in seqs) == m
    exp = expected(owner, group_of_cases(["d"]))
    for route in ("host", "device"):
        got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, route)
        compare(got, exp, owner)
        check_counts(stats, route, n_sent, owner, exp)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("W", sorted(E.PROMOTIONS))
def test_promotion(monkeypatch, W, route):
    """pairs of W words each and 2 W together: the device files their tiles under 2 W, the host cuts them and stays in W"""
    case, = [c for c in E.cases("i") if c.tile["own_w"] == W]
    seqs, q, t, k, owner = E.flatten([case])
    exp = expected(owner, group_of_cases(["i"]))
    got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, route)
    compare(got, exp, owner)
    check_counts(stats, route, n_sent, owner, exp)
    loc = {w: stats["locate_tiles_w%d" % w] for w in CLASSES}
    if route == "host":
        assert loc[W] == len(E.host_tiles(case)) >= 2 and sum(loc.values()) == loc[W]
    else:
        assert loc[2 * W] > 0 and sum(loc.values()) == loc[W] + loc[2 * W] == n_sent // 64          # one bucket (query, W) in runs of 64
        assert loc[W] <= 1                               # (a run that drew one kind of pair only stays in W: one in 2^63)


def test_fall_back_from_device_tiles_to_host_tiles(monkeypatch):
    """2048 pairs of one query that fit 512 diagonals each and not together: the device route gives up, the host's greedy cut separates them"""
    rng = random.Random(512)
    b = E.body(rng, 300)
    seqs = [b, "T" * 190 + E.plant(b, 3, "sub") + "T" * 190, E.plant(b, 5, "del")]
    q, t, k = [0] * 2048, [1, 2] * 1024, [20, 200] * 1024
    assert E.words(E.rows(380, 20)) == E.words(E.rows(-5, 200)) == 8 and E.words(E.rows(380, 200)) == 0
    got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, "device")
    assert got[:2] == [E.oracle_row(b, seqs[1], 20), E.oracle_row(b, seqs[2], 200)] == [[3, 190, 489, 0, 0], [5, 0, 294, 0, 0]]
    assert got == got[:2] * 1024
    assert stats["route"] == 0 and stats["retried_host"] == 1 and stats["pairs"] == stats["need_kernel"] == stats["hits"] == 2048
    # (the greedy cut starts a LOCATE tile wherever the kind changes in the shuffled list; the hits are classed by 2 k + 1: 41 and 401)
    assert 2 * 1024 // 64 < stats["locate_tiles_w8"] <= 2048 and stats["locate_tiles_w1"] == stats["locate_tiles_w2"] == stats["locate_tiles_w4"] == 0
    assert stats["finish_tiles_w1"] == stats["finish_tiles_w8"] == 1024 // 64


MIXED = tuple("abcdefghi")


@pytest.fixture(scope="module")
def mixed():
    group_of = group_of_cases(MIXED)
    case_list = [c for g in MIXED for c in E.cases(g)]
    random.Random(77).shuffle(case_list)                 # the classes interleaved in the store and in the pair list
    seqs, q, t, k, owner = E.flatten(case_list, bystander=BYSTANDER)
    return seqs, q, t, k, owner, expected(owner, group_of)


@pytest.mark.parametrize("route", ["host", "device"])
def test_all_groups_in_one_call(monkeypatch, mixed, route):
    seqs, q, t, k, owner, exp = mixed
    got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, route)
    compare(got, exp, owner)
    check_counts(stats, route, n_sent, owner, exp)
    assert all(stats["locate_tiles_w%d" % w] > 0 and stats["finish_tiles_w%d" % w] > 0 for w in CLASSES)


def test_wide_entry_gives_the_same_rows(monkeypatch, mixed):
    seqs, q, t, k, owner, exp = mixed
    for route in ("host", "device"):
        got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, route, wide=True)
        compare(got, exp, owner)
        assert stats["route"] == (0 if route == "host" else 1) and stats["pairs"] == n_sent          # no pair beyond 512 diagonals: the call is isocon_hw_pairs


def test_path_entry_gives_the_same_rows(monkeypatch, mixed):
    """SeqStore.hw_path_pairs: its rows are those of the wide entry, so the oracle's"""
    seqs, q, t, k, owner, exp = mixed
    got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, "host", method="hw_path_pairs")
    compare(got, exp, owner)
    for W in (1, 2):                                     # ... and past the finish grid, tiles built on the device
        seqs, q, t, k, owner = E.flatten(E.cases("j%d" % W))
        exp = expected(owner, group_of_cases(["j%d" % W]))
        got, stats, n_sent = hw_call(monkeypatch, seqs, q, t, k, "device", method="hw_path_pairs")
        compare(got, exp, owner)
        assert stats["route"] == 1 and stats["finish_tiles_w%d" % W] > stats["finish_grid_w%d" % W] > 0
