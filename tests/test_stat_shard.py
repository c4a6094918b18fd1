"""CPU: who owns which edge of a round of hypothesis tests (isocon_amd.dist.shard_edges), and two ranks over gloo that share a round
(hypothesis_test_module.do_statistical_tests_per_edge) on the host tables with the oracle's alignments: every rank's dict is the
single-process dict, key order and float bits included.  The device route: tests/test_gpu_stat_shard.py."""
import itertools
import random

import pytest

import stat_shard_cases as SC
from isocon_amd import dist as D


def _edge_list(n, seed):
    """n edges of a few candidates each pointing to several references, skewed weights (one edge in eight is a hundred times the others)"""
    rng = random.Random(seed)
    pool = ["%s%d" % (rng.choice("ct"), k) for k in range(max(4, n))]
    edges = []
    for c, t in itertools.product(pool[: max(2, n // 3 + 1)], pool):
        if c != t and len(edges) < n:
            edges.append((c, t))
    assert len(edges) == n
    rng.shuffle(edges)
    return edges, [rng.randint(1, 9) * (100 if rng.random() < 0.125 else 1) for _ in edges]


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_every_edge_has_one_owner_in_contiguous_balanced_runs(world):
    for n in sorted({0, 1, max(world - 1, 0), world, 50}):
        edges, weights = _edge_list(n, 100 * world + n)
        runs = D.shard_edges(edges, weights, world)
        assert len(runs) == world
        canonical = sorted(edges, key=lambda e: (str(e[0]), str(e[1])))
        assert [e for run in runs for e in run] == canonical          # every edge once; each run a contiguous piece of the canonical list
        weight_of = dict(zip(edges, weights))
        if n:
            assert max(sum(weight_of[e] for e in run) for run in runs) <= sum(weights) / world + max(weights)
        # the order in which the edges come in does not matter
        rng = random.Random(n)
        for _ in range(3):
            both = list(zip(edges, weights))
            rng.shuffle(both)
            assert D.shard_edges([e for e, _ in both], [w for _, w in both], world) == runs
            assert D.edge_digest([e for e, _ in both], [w for _, w in both]) == D.edge_digest(edges, weights)
        if n:
            assert D.edge_digest(edges, [weights[0] + 1] + weights[1:]) != D.edge_digest(edges, weights)
            assert D.edge_digest(edges[1:], weights[1:]) != D.edge_digest(edges, weights)


def test_the_edges_of_one_candidate_stay_together_when_weights_are_even():
    """contiguity in (c, t) order: with 3 edges per c and equal weights, at most world - 1 candidates are split between two ranks"""
    edges = [("c%d" % k, "t%d" % j) for k in range(20) for j in range(3)]
    runs = D.shard_edges(edges, [5] * len(edges), 4)
    owners = {}
    for r, run in enumerate(runs):
        for c, _ in run:
            owners.setdefault(c, set()).add(r)
    assert sum(len(v) > 1 for v in owners.values()) <= 3 and all(len(v) <= 2 for v in owners.values())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_two_ranks_equal_the_single_process(tmp_path, fastq):
    ranks = SC.run_ranks(2, "equal", tmp_path, cpu=True, fastq=fastq, orders=True)
    for got in ranks:
        assert SC.same_result(got["shared"], got["alone"]) and SC.same_result(got["replicated"], got["alone"])
        assert [(c, t) for c, row in got["shared"].items() for t in row] == got["edges"]          # this rank's own order
        assert sum(v[0] not in (0.0, 1.0) for row in got["alone"].values() for v in row.values()) >= 3
    assert ranks[0]["edges"] != ranks[1]["edges"] and sorted(ranks[0]["edges"]) == sorted(ranks[1]["edges"])
    live = ranks[0]["live"]
    assert all(0 < got["moved"]["edges_owned"] < live and got["moved"]["edges_total"] == live and got["moved"]["rounds"] == 1 for got in ranks)
    assert sum(got["moved"]["edges_owned"] for got in ranks) == live
    assert all(got["moved"]["gather_bytes"] > 0 and got["moved_replicated"]["rounds"] == 0 for got in ranks)


@pytest.mark.timeout(300)
def test_two_ranks_raise_what_the_first_edge_raises(tmp_path):
    ranks = SC.run_ranks(2, "raising", tmp_path, cpu=True, second=True)
    assert ranks[0]["planted"] == ranks[1]["planted"] and len(ranks[0]["planted"]) == 2
    assert sorted(ranks[0]["owner"][e] for e in ranks[0]["planted"]) == [0, 1]
    assert ranks[0]["first"] != ranks[1]["first"]
    for got in ranks:
        assert got["shared"][0] == got["planted"][got["first"]] and got["shared"] == got["alone"]
