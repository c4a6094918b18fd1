"""The argument behind the table of seed pairs (NNSeedKnown, csrc/nn_list.hpp), as a small model on the CPU.

The search's update rule for a pair (a, b) of distance d, as k_ed_lanes<true> carries it out: k = min(63, max(best[a], best[b])); the
alignment answers r = d if d <= k and nothing otherwise; an end e takes r if r <= best[e] (best[e] = r, the hit (e, partner, r) joins the
list).  At the end a hit is an edge iff its distance equals its row's final bound, duplicates dropped (nn_fin_valid, k_fin_rows).

The seed pass runs first and is finished before the main pass meets its first pair.  best[] only decreases, so a seed pair's k in the seed
pass is at least its k in the main pass: aligning it a second time can neither find something the first run missed nor change a bound, and
the hit it would append is a duplicate.  The model runs the main pass with and without the seed pairs, in shuffled orders, on random
symmetric distance matrices with many ties: bounds and rows must be equal.  Two mutants show that the comparison can fail: a table that
holds a pair the seed pass never aligned, and a seed pass that aligned its pairs under a smaller k than the main pass would have used.
"""
import random

import pytest

INF = 0x3FFFFFFF


def random_case(rng):
    """(n, distance matrix as a dict of rows, seed pairs): a few clusters, distances from a handful of values so that ties are the rule, some
    beyond the 63 of the band"""
    n = rng.randrange(40, 201)
    n_clusters = rng.randrange(2, 6)
    cluster = [rng.randrange(n_clusters) for _ in range(n)]
    near, far = [rng.randrange(1, 9) for _ in range(4)], [rng.randrange(30, 90) for _ in range(4)]
    d = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            d[a][b] = d[b][a] = rng.choice(near if cluster[a] == cluster[b] else far)
    # seeds: up to four partners per entry by a noisy estimate of the distance (the q-gram bounds' stand-in), proposed from one side
    seeds = set()
    for a in range(n):
        others = sorted((x for x in range(n) if x != a), key=lambda x: d[a][x] + rng.randrange(0, 12))
        for b in others[:rng.randrange(0, 5)]:
            seeds.add((min(a, b), max(a, b)))
    return n, d, sorted(seeds)


def align(best, hits, d, a, b, k_of=max):
    k = min(63, k_of(best[a], best[b]))
    if d[a][b] > k:
        return
    r = d[a][b]
    for e, other in ((a, b), (b, a)):
        if r <= best[e]:
            best[e] = r
            hits.append((e, other, r))


def graph(n, best, hits):
    rows = [set() for _ in range(n)]
    for e, other, r in hits:
        if r == best[e]:
            rows[e].add(other)          # (a set: duplicates dropped)
    return best, [sorted(r) for r in rows]


def search(n, d, seeds, order_rng, skip, known=None, seed_k=max):
    """seed pass over `seeds`, then the main pass over every pair in a shuffled order; skip: the main pass leaves out the pairs in `known`
    (default: the seed pairs themselves)"""
    best, hits = [INF] * n, []
    seeds = list(seeds)
    order_rng.shuffle(seeds)
    for a, b in seeds:
        align(best, hits, d, a, b, seed_k)
    known = set(seeds) if known is None else known
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    order_rng.shuffle(pairs)
    for a, b in pairs:
        if skip and (a, b) in known:
            continue
        align(best, hits, d, a, b)
    return graph(n, best, hits)


CASES = list(range(12))


@pytest.mark.parametrize("case", CASES)
def test_skipping_the_seed_pairs_changes_nothing(case):
    rng = random.Random(1000 + case)
    n, d, seeds = random_case(rng)
    assert seeds
    reference = None
    for order in range(4):
        with_all = search(n, d, seeds, random.Random(order), skip=False)
        skipped = search(n, d, seeds, random.Random(order), skip=True)
        assert skipped == with_all
        # (the graph is no function of the order either: exact arg-min sets)
        reference = reference or with_all
        assert with_all == reference
    assert any(reference[1])


def test_a_table_with_a_pair_that_never_ran_is_caught():
    """mutant 1: the table also holds pairs the seed pass did not align"""
    differs = 0
    for case in CASES:
        rng = random.Random(1000 + case)
        n, d, seeds = random_case(rng)
        extra = {(a, b) for a in range(n) for b in range(a + 1, n) if rng.random() < 0.05}
        good = search(n, d, seeds, random.Random(0), skip=False)
        bad = search(n, d, seeds, random.Random(0), skip=True, known=set(seeds) | extra)
        differs += bad != good
    assert differs > 0


def test_a_seed_pass_under_a_smaller_k_is_caught():
    """mutant 2: the seed pass aligned under k = min of the two bounds -- below what the main pass would use -- and its pairs are skipped all the same"""
    differs = 0
    for case in CASES:
        rng = random.Random(1000 + case)
        n, d, seeds = random_case(rng)
        good = search(n, d, seeds, random.Random(0), skip=False)
        bad = search(n, d, seeds, random.Random(0), skip=True, seed_k=min)
        differs += bad != good
    assert differs > 0
