"""GPU: the hypothesis tests of a round shared between the ranks of a process group (hypothesis_test_module._shared_rows, dist.shard_edges)
on the device route: every rank's dict is the dict the same process computed alone before the group existed -- keys, order, float bits --
while each rank sent only its own edges through isocon_edge_variants and isocon_raghavan_bound; few and no live edges, ranks that hold the
edges in different orders or hold different edges, tests that raise, and the whole pipeline with its result files and per-rank table uploads.
The ranks share the one GPU and talk over gloo; scenarios and inputs: tests/stat_shard_cases.py."""
import pytest

import stat_shard_cases as SC
from isocon_amd import dist as D

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_each_rank_tests_its_own_edges_and_holds_the_single_process_result(tmp_path, fastq):
    """(odd ranks hold the graph in the opposite order: each rank gets ITS single-process dict)"""
    ranks = SC.run_ranks(2, "equal", tmp_path, fastq=fastq, orders=True)
    live = ranks[0]["live"]
    assert live >= 8 and ranks[0]["edges"] != ranks[1]["edges"] and sorted(ranks[0]["edges"]) == sorted(ranks[1]["edges"])
    for got in ranks:
        assert SC.same_result(got["shared"], got["alone"]) and SC.same_result(got["replicated"], got["alone"])
        assert [(c, t) for c, row in got["shared"].items() for t in row] == got["edges"]
        assert sum(v[0] not in (0.0, 1.0) for row in got["alone"].values() for v in row.values()) >= 3
        moved, replicated = got["moved"], got["moved_replicated"]
        print("live edges %d; sharded: %r; stat_all_edges: %r" % (live, moved, replicated))
        # the device saw this rank's edges only: fewer than there are ...
        assert 0 < moved["edges"] < live and 0 < moved["tests"] < live
        assert moved.get("rounds") == 1 and moved["edges_owned"] == moved["edges"] and moved["edges_total"] == live and moved["gather_bytes"] > 0
        # ... and all of them under ISOCON_DEBUG_VARIANT=stat_all_edges
        assert replicated["edges"] == live and replicated["tests"] == live and replicated["rounds"] == 0 and replicated["edges_owned"] == 0
        assert 0 < moved["rows"] < replicated["rows"]
    # ... that sum to all live edges over the ranks
    assert sum(got["moved"]["edges"] for got in ranks) == live and sum(got["moved"]["tests"] for got in ranks) == live
    assert sum(got["moved"]["edges_owned"] for got in ranks) == live


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,keep", [(4, 3), (2, 1), (2, 0)], ids=["4_ranks_3_edges", "2_ranks_1_edge", "2_ranks_no_edge"])
def test_fewer_live_edges_than_ranks(tmp_path, world, keep):
    ranks = SC.run_ranks(world, "equal", tmp_path, fastq=True, keep=keep)
    assert all(got["live"] == keep for got in ranks)
    for got in ranks:
        assert SC.same_result(got["shared"], got["alone"])
        rows = [row for inner in got["shared"].values() for row in inner.values()]
        assert len(rows) == 12 and sum(row == (1.0, 1.0, 0, 0, "") for row in rows) == 12 - keep
        assert got["moved"]["rounds"] == 1 and got["moved"]["edges_total"] == keep
        assert got["moved"]["edges"] == got["moved"]["edges_owned"] <= 1          # (three edges over four ranks: nobody has two)
    assert sum(got["moved"]["edges_owned"] for got in ranks) == keep
    assert sum(got["moved"]["edges_owned"] == 0 for got in ranks) == world - keep          # ranks without an edge went through the round too


@pytest.mark.timeout(300)
def test_ranks_with_different_edges_are_rejected(tmp_path):
    ranks = SC.run_ranks(2, "different_sets", tmp_path)
    for raised in ranks:
        assert raised is not None and raised[0] == "RuntimeError" and "digest mismatch" in raised[1]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("second", [False, True], ids=["one_edge_raises", "two_edges_raise"])
def test_every_rank_raises_what_its_first_raising_edge_raises(tmp_path, second):
    ranks = SC.run_ranks(2, "raising", tmp_path, second=second)
    planted, owner = ranks[0]["planted"], ranks[0]["owner"]
    assert ranks[1]["planted"] == planted and sorted(owner[e] for e in planted) == ([0, 1] if second else [1])
    assert "SystemExit" in planted.values() and len(set(planted.values())) == len(planted)
    for got in ranks:
        assert got["shared"] is not None and got["shared"][0] == planted[got["first"]]
        assert got["alone"] == got["shared"]          # (type and text)
    # the SystemExit comes from the device's answer: rank 1's table set took its qualities and was asked about them
    assert ranks[1]["moved"]["quality_attach_calls"] == 1 and ranks[1]["moved"]["quality_calls"] >= 1
    if second:
        assert ranks[0]["first"] != ranks[1]["first"] and ranks[0]["shared"][0] != ranks[1]["shared"][0]
    else:
        assert [got["shared"][0] for got in ranks] == ["SystemExit", "SystemExit"]


@pytest.fixture(scope="module")
def pipeline_ranks(tmp_path_factory):
    return SC.run_ranks(2, "pipeline", tmp_path_factory.mktemp("pipeline"), files_dir=str(tmp_path_factory.mktemp("pipeline_files")), **SC.PIPELINE)


@pytest.mark.timeout(300)
def test_pipeline_files_are_the_single_process_files_on_every_rank(pipeline_ranks):
    names = sorted(pipeline_ranks[0]["alone"]["files"])
    assert "final_candidates.fa" in names and "cluster_info.tsv" in names
    assert sum(f.startswith("p_values_") for f in names) >= 2          # at least two rounds
    assert max(len(got["shared"]["rounds"]) for got in pipeline_ranks) >= 2
    for got in pipeline_ranks:
        assert sorted(got["shared"]["files"]) == names
        for f in names:
            assert got["shared"]["files"][f] == got["alone"]["files"][f] == pipeline_ranks[0]["alone"]["files"][f], f
        assert len(got["alone"]["files"]["final_candidates.fa"]) > 0


@pytest.mark.timeout(300)
def test_pipeline_ranks_upload_their_own_tables(pipeline_ranks):
    """rows uploaded to the device tables: each rank fewer than the single process; together at most its rows plus, ONCE, the rows of every
    table that both ranks need -- found here from shard_edges itself.  A table is a candidate's reads in one version (the scenario counts a
    new version whenever the cache would build the table anew); a rank needs it if an edge of its share has the candidate while that version
    stands, in whichever round: the process that tests all edges uploads such a table once, two ranks that both need it twice."""
    alone = pipeline_ranks[0]["alone"]["rows"]
    assert alone > 0 and all(got["alone"]["rows"] == alone for got in pipeline_ranks)
    rounds = pipeline_ranks[0]["shared"]["rounds"]
    assert all(got["shared"]["rounds"] == rounds for got in pipeline_ranks) and pipeline_ranks[0]["alone"]["rounds"] == rounds
    rows_of, needed_by = {}, ({}, {})          # (acc, version) -> rows; per rank the tables it needs
    for live, weights, tables in rounds:
        for r, share in enumerate(D.shard_edges(live, weights, 2)):
            for acc in {acc for e in share for acc in e}:
                rows_of[(acc, tables[acc][1])] = needed_by[r][(acc, tables[acc][1])] = tables[acc][0]
    allowance = sum(rows_of[t] for t in needed_by[0].keys() & needed_by[1].keys())
    figures = [got["shared"]["rows"] for got in pipeline_ranks]
    print("rows uploaded: alone %d (all tables in all versions: %d), per rank %r (their tables: %r), of tables that both ranks need %d"
          % (alone, sum(rows_of.values()), figures, [sum(n.values()) for n in needed_by], allowance))
    # the cache does what the versions say: one upload per table and process that needs it
    assert alone == sum(rows_of.values()) and figures == [sum(n.values()) for n in needed_by]
    assert 0 < allowance < alone
    assert all(0 < x < alone for x in figures)
    assert sum(figures) <= alone + allowance
