"""Inputs, ranks and scenarios of the tests of the sharded hypothesis tests (hypothesis_test_module._shared_rows), shared by
tests/test_stat_shard.py (CPU: host tables, the oracle's alignments) and tests/test_gpu_stat_shard.py (the device route; the ranks share
the one GPU and talk over gloo).  A scenario runs in every rank of a freshly spawned group: it makes its input from a seed, runs what it
needs of the single-process path BEFORE the group exists, starts the group, runs the sharded path and hands back what the test compares."""
import datetime
import os
import pickle
import random
import socket
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class _Params(object):
    max_phred_q_trusted = 43


class _NotHeld(str):
    """a record sequence that equals its read and still says that it does not hold it (as readtab_quality_cases.SeqAt lies about where):
    the hoisted comparison with X passes, the edge's own test raises ValueError"""

    def index(self, *_):
        raise ValueError("substring not found")


def partition(seed=5, n_t=4, n_c=12, shared_t=True, cc_edges=True):
    """(C, read partition, graph c -> t, X, ccs): n_c candidates, each a mutated copy of one of n_t references (shared_t: several candidates
    point to one t; else every candidate has a t of its own) and, with cc_edges, also pointing to the candidate made n_t before it from the
    same t.  Every candidate differs from its t at inner bases, so every edge has variants.  Accessions are not zero-padded ("c10" < "c2"): the
    canonical order is not the order of the dicts."""
    from oracle import oracle as O
    import readtab_quality_cases as QC
    rng = random.Random(seed)

    def mut(b, n, lo=0):
        v = list(b)
        for _ in range(n):
            p = rng.randrange(lo, len(v) - lo)
            r = rng.random()
            if r < 0.5:
                v[p] = rng.choice([x for x in "ACGT" if x != v[p]])
            elif r < 0.75:
                del v[p]
            else:
                v.insert(p, rng.choice("ACGT"))
        return "".join(v)

    def reads_of(acc, seq, n):
        return {"r_%s_%d" % (acc, k): O.parasail_alignment(seq, mut(seq, rng.randint(0, 3)), 0, 0)[2] for k in range(n)}

    C, part, graph = {}, {}, {}
    for k in range(n_c):
        j = k % n_t if shared_t else k
        if "t%d" % j not in C:
            C["t%d" % j] = "".join(rng.choice("AACGTT") for _ in range(rng.randint(70, 130)))
            part["t%d" % j] = reads_of("t%d" % j, C["t%d" % j], rng.randint(3, 8))
        while True:
            c = mut(C["t%d" % j], rng.randint(1, 3), lo=10)
            if c not in C.values():
                break
        C["c%d" % k] = c
        part["c%d" % k] = reads_of("c%d" % k, c, rng.randint(3, 6))
        graph["c%d" % k] = {"t%d" % j: 1}
        if cc_edges and shared_t and k >= n_t:
            graph["c%d" % k]["c%d" % (k - n_t)] = 1
    X = {acc: v[1].replace("-", "") for ra in part.values() for acc, v in ra.items()}
    ccs = {acc: QC.record(rng, acc, x, prefix="", suffix="") for acc, x in X.items()}
    return C, part, graph, X, ccs


def edges_of(graph):
    return [(c, t) for c in graph for t in graph[c]]


def live_and_weights(graph, part):
    live = [(c, t) for c, t in edges_of(graph) if len(part[c]) + len(part[t]) > 0]
    return live, [1 + len(part[c]) + len(part[t]) for c, t in live]


def reordered(graph):
    """the same graph with its rows and every row's columns in the opposite order"""
    return {c: dict(reversed(list(graph[c].items()))) for c in reversed(list(graph))}


def bits(p_values):
    """a result with every p-value as its eight bytes, rows and columns in dict order"""
    return [(c, [(t, struct.pack("<d", row[0])) + tuple(row[1:]) for t, row in inner.items()]) for c, inner in p_values.items()]


def same_result(a, b):
    return list(a.items()) == list(b.items()) and [list(x.items()) for x in a.values()] == [list(x.items()) for x in b.values()] and bits(a) == bits(b)


def _H():
    from isocon_amd import hypothesis_test_module as H
    return H


def _round(graph, C, X, part, ccs):
    H = _H()
    H.clear_tables()          # (every run builds and uploads its own tables)
    return H.do_statistical_tests_per_edge(graph, C, X if ccs else {}, part, ccs, _Params())


def _counters():
    H = _H()
    out = {"edges": H.EDGE_VARIANT_STATS["edges"], "tests": H.BOUND_STATS["tests"], "rows": H.DEVICE_STATS["rows_uploaded"],
           "quality_attach_calls": H.DEVICE_STATS["quality_attach_calls"], "quality_calls": H.DEVICE_STATS["quality_calls"]}
    out.update(getattr(H, "SHARD_STATS", {}))
    return out


def _counted(fn):
    before = _counters()
    out = fn()
    return out, {k: v - before.get(k, 0) for k, v in _counters().items()}


def _outcome(fn):
    """(result, None) or (None, (type name, text)) of what fn raises -- SystemExit is among what a test raises"""
    try:
        return fn(), None
    except (Exception, SystemExit) as exc:
        return None, (type(exc).__name__, str(exc))


def scenario_equal(rank, world, start, fastq=False, keep=None, orders=False):
    """alone (before the group), sharded, and replicated under ISOCON_DEBUG_VARIANT=stat_all_edges, with what the counters moved by.
    keep: only the first `keep` edges keep their reads (every candidate has a t of its own here); orders: odd ranks hold the graph reversed"""
    C, part, graph, X, ccs = partition(shared_t=keep is None)
    if keep is not None:
        for c, t in edges_of(graph)[keep:]:
            part[c], part[t] = {}, {}
    if orders and rank % 2:
        graph = reordered(graph)
    ccs = ccs if fastq else None
    run = lambda: _round(graph, C, X, part, ccs)  # noqa: E731
    alone = run()
    start()
    shared, moved = _counted(run)
    switches = os.environ.get("ISOCON_DEBUG_VARIANT", "")
    os.environ["ISOCON_DEBUG_VARIANT"] = ",".join(x for x in (switches, "stat_all_edges") if x)
    replicated, moved_replicated = _counted(run)
    os.environ["ISOCON_DEBUG_VARIANT"] = switches
    live, weights = live_and_weights(graph, part)
    return {"alone": alone, "shared": shared, "replicated": replicated, "moved": moved, "moved_replicated": moved_replicated, "live": len(live),
            "edges": edges_of(graph)}


def scenario_different_sets(rank, world, start):
    """rank 1 holds one edge less"""
    C, part, graph, X, ccs = partition()
    if rank == 1:
        del graph[next(iter(graph))]
    start()
    return _outcome(lambda: _round(graph, C, X, part, None))[1]


def scenario_raising(rank, world, start, second=False):
    """The first edge of rank 1's share (dist.shard_edges) gets reads of c whose quality records end before the read: the records attach to
    the device tables, the device's answer raises SystemExit.  With `second` the first edge of rank 0's share gets reads of c whose records
    say that they do not hold them (ValueError, on the host tables: such a set attaches nothing), and rank 1 holds the graph reversed.
    moved: what the sharded round moved this rank's counters by."""
    import readtab_quality_cases as QC
    from isocon_amd import dist as D
    C, part, graph, X, ccs = partition(cc_edges=False)          # (a candidate's reads are looked at by its one edge only)
    live, weights = live_and_weights(graph, part)
    shares = D.shard_edges(live, weights, world)
    rng = random.Random(1)

    def plant(records, e, how):
        out = dict(records)
        for acc in part[e[0]]:
            if how == "beyond":
                out[acc] = QC.record(rng, acc, X[acc], prefix="", suffix="", at=len(X[acc]) + 5)
            else:
                out[acc] = QC.CCS(acc, _NotHeld(X[acc]), list(records[acc].qual), 1)
        return out

    planted_at = {shares[1][0]: "SystemExit"}
    records = plant(ccs, shares[1][0], "beyond")
    if second:
        planted_at[shares[0][0]] = "ValueError"
        records = plant(records, shares[0][0], "not_held")
        if rank == 1:
            graph = reordered(graph)
    first = min(planted_at, key=edges_of(graph).index)
    alone = _outcome(lambda: _round(graph, C, X, part, records))[1]
    start()
    (_, shared), moved = _counted(lambda: _outcome(lambda: _round(graph, C, X, part, records)))
    return {"planted": planted_at, "owner": {e: r for r in range(world) for e in shares[r]}, "first": first, "alone": alone, "shared": shared,
            "moved": moved}


def scenario_pipeline(rank, world, start, files_dir=None, seed=7, n_reads=300, fastq=False):
    """find_candidate_transcripts + stat_filter_candidates on a small synthetic read set, alone and in the group: the result files, the rows
    uploaded, and of every round of a run its live edges, their weights and, per candidate of a live edge, (reads, version): the version of a
    candidate's read table changes exactly when the table cache (hypothesis_test_module._tables_for) would build it anew -- another dict, or
    another alignment tuple in it"""
    import numpy as np
    from isocon_amd import isocon_get_candidates as IGC
    from isocon_amd import isocon_statistical_test as IST
    from isocon_amd import synth
    H = _H()
    accs, seqs, _ = synth.make_reads(n_reads, 350, 4, seed)
    rounds, seen = [], {}          # seen: acc -> (its dict, its alignment tuples, version) when last recorded (kept alive: identities stay taken)
    original = H.do_statistical_tests_per_edge

    def recording(graph, C, X, part, ccs_dict, params):
        live, weights = live_and_weights(graph, part)
        tables = {}
        for acc in dict.fromkeys(acc for e in live for acc in e):
            ra, stamp, last = part[acc], list(part[acc].values()), seen.get(acc)
            if last is None or last[0] is not ra or len(last[1]) != len(stamp) or not all(a is b for a, b in zip(last[1], stamp)):
                last = seen[acc] = (ra, stamp, 0 if last is None else last[2] + 1)
            tables[acc] = (len(ra), last[2])
        rounds.append((live, weights, tables))
        return original(graph, C, X, part, ccs_dict, params)

    def run(tag):
        tmp = os.path.join(files_dir, "rank%d_%s" % (rank, tag))
        os.makedirs(tmp)
        read_file = os.path.join(tmp, "reads.fq" if fastq else "reads.fa")
        rq = np.random.default_rng(1)
        with open(read_file, "w") as fh:
            for a, s in zip(accs, seqs):
                if fastq:
                    fh.write("@%s\n%s\n+\n%s\n" % (a, s, (rq.integers(5, 60, len(s)) + 33).astype(np.uint8).tobytes().decode()))
                else:
                    fh.write(">%s\n%s\n" % (a, s))

        class P(object):
            nr_cores = 1; neighbor_search_depth = 2 ** 32; verbose = False; develop_logfile = None; logfile = None; min_exon_diff = 20  # noqa: E702
            ignore_ends_len = 15; min_candidate_support = 2; is_fastq = fastq; ccs = None; outfolder = tmp  # noqa: E702
            p_value_threshold = 0.01; min_test_ratio = 5; max_phred_q_trusted = 43  # noqa: E702

        del rounds[:]
        seen.clear()
        before = _counters()
        cand_file, rp, to_realign = IGC.find_candidate_transcripts(read_file, P)
        IST.stat_filter_candidates(read_file, cand_file, rp, to_realign, P)
        names = sorted(f for f in os.listdir(tmp) if f in ("final_candidates.fa", "cluster_info.tsv") or f.startswith("p_values_"))
        return {"files": {f: open(os.path.join(tmp, f), "rb").read() for f in names}, "rows": _counters()["rows"] - before["rows"], "rounds": list(rounds)}

    H.do_statistical_tests_per_edge = recording
    try:
        alone = run("alone")
        start()
        return {"alone": alone, "shared": run("shared")}
    finally:
        H.do_statistical_tests_per_edge = original


PIPELINE = {"seed": 7, "n_reads": 300, "fastq": True}          # 300 reads of 4 isoforms of ~350 bases: seven rounds, four of them with tests (22, 10, 5 and 2 edges)
SCENARIOS = {"equal": scenario_equal, "different_sets": scenario_different_sets, "raising": scenario_raising, "pipeline": scenario_pipeline}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank(rank, world, port, name, out_dir, cpu, kwargs):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ISOCON_DIST_BACKEND="gloo", ISOCON_GPU_DEVICE="0",
                      ISOCON_DEBUG_VARIANT="stat_host_tables" if cpu else "")
    import torch.distributed as dist
    if cpu:          # the host tables on the oracle's alignments: no device call in a round
        import isocon_amd.SW_alignment_module as SWM
        from test_stat_test import oracle_align_pairs
        SWM._align_pairs = oracle_align_pairs

    def start():
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))

    try:
        result = SCENARIOS[name](rank, world, start, **kwargs)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    with open(os.path.join(out_dir, "rank%d.pkl" % rank), "wb") as fh:
        pickle.dump(result, fh)


def run_ranks(world, name, out_dir, cpu=False, limit=150, **kwargs):
    """the scenario in `world` freshly spawned ranks; [what rank r returned].  A rank that dies ends the others; so does the limit."""
    import torch.multiprocessing as mp
    out_dir = str(out_dir)
    ctx = mp.spawn(_rank, args=(world, _free_port(), name, out_dir, cpu, kwargs), nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5):          # (returns as soon as a rank ends; raises what a rank raised, after ending the others)
            if time.monotonic() > deadline:
                raise TimeoutError("the ranks of scenario %r did not finish within %d s" % (name, limit))
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    out = []
    for r in range(world):
        with open(os.path.join(out_dir, "rank%d.pkl" % r), "rb") as fh:
            out.append(pickle.load(fh))
    return out
