"""Wall time of the whole pipeline (find_candidate_transcripts + stat_filter_candidates) on synthetic CCS reads, with a
breakdown of the statistical-test phase.  Usage: python scripts/time_full_pipeline.py [n_reads] [length] [isoforms] [ont|ccs] [fastq]
The SHA-256 of every result file is printed; ISOCON_KEEP_RESULTS=<directory> also keeps copies of them there (for a cmp between runs).
One process per GPU: under `python -m torch.distributed.run --nproc-per-node N` (WORLD_SIZE in the environment) the process group is started
as in scripts/spmd_pipeline_check.py (backend from ISOCON_DIST_BACKEND, default nccl); rank 0 prints the lines above, every rank its share of
the hypothesis tests, the rows it uploaded to the device read tables, their bytes and the digests of its result files."""
import cProfile, hashlib, os, pstats, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rank, dist = 0, None
if "WORLD_SIZE" in os.environ:
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("ISOCON_GPU_DEVICE", str(local_rank))
    import torch
    import torch.distributed as dist
    if os.environ.get("ISOCON_DIST_BACKEND", "nccl") == "nccl":
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend=os.environ["ISOCON_DIST_BACKEND"])
    rank = dist.get_rank()
say = print if rank == 0 else (lambda *a, **k: None)
from isocon_amd import synth
from isocon_amd import isocon_get_candidates as IGC
from isocon_amd import isocon_statistical_test as IST
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
L = int(sys.argv[2]) if len(sys.argv) > 2 else 2500
iso = int(sys.argv[3]) if len(sys.argv) > 3 else 10
if len(sys.argv) > 4 and sys.argv[4] == "ont":      # ONT error profile (6 %), two gene families of mixed length
    accs, seqs, isoforms = synth.make_reads(n, 0, iso, 50001, profile=synth.ONT_PROFILE, families=2, length_range=(1000, L))
else:
    accs, seqs, isoforms = synth.make_reads(n, L, iso, 30001)
with tempfile.TemporaryDirectory() as tmp:
    fastq = "fastq" in sys.argv[4:]           # FASTQ input with random base qualities: the tests then use them
    rf = os.path.join(tmp, "reads.fq" if fastq else "reads.fa")
    with open(rf, "w") as fh:
        if fastq:
            import numpy as np
            rq = np.random.default_rng(1)
            for a, s in zip(accs, seqs): fh.write("@%s\n%s\n+\n%s\n" % (a, s, (rq.integers(5, 60, len(s)) + 33).astype(np.uint8).tobytes().decode()))
        else:
            for a, s in zip(accs, seqs): fh.write(">%s\n%s\n" % (a, s))
    class Out:
        def write(self, x):
            if rank == 0: sys.stdout.write(x); sys.stdout.flush()
    class P: nr_cores = 1; neighbor_search_depth = 2 ** 32; verbose = False; develop_logfile = None; logfile = Out(); min_exon_diff = 20
    P.ignore_ends_len = 15; P.min_candidate_support = 2; P.is_fastq = fastq; P.ccs = None; P.outfolder = tmp
    P.p_value_threshold = 0.01; P.min_test_ratio = 5; P.max_phred_q_trusted = 43
    t = time.time(); cand_file, rp, to_realign = IGC.find_candidate_transcripts(rf, P); t1 = time.time() - t
    ncand = sum(1 for l in open(cand_file) if l.startswith(">"))
    say("find_candidate_transcripts: %.1f s -> %d candidates, %d reads assigned, %d to realign" % (t1, ncand, sum(len(v) for v in rp.values()), len(to_realign)), flush=True)
    import numpy as np
    from isocon_amd import end_invariant_functions as END
    cl = np.sort(np.array([len(l.strip()) for l in open(cand_file) if not l.startswith(">")], dtype=np.int64))
    say("candidate-vs-candidate infix alignments (window 10 + 2 x 15): %d pairs" % len(END._window_pairs(cl, 0, len(cl), 40, 2 ** 32)[0]), flush=True)
    from isocon_amd import hypothesis_test_module as H
    TABLE_BYTES, per_edge = [0], H.do_statistical_tests_per_edge
    def per_edge_and_bytes(*a):
        out = per_edge(*a); TABLE_BYTES[0] = max(TABLE_BYTES[0], H.device_table_bytes()); return out
    H.do_statistical_tests_per_edge = per_edge_and_bytes
    pr = cProfile.Profile(); t = time.time(); pr.enable()
    C = IST.stat_filter_candidates(rf, cand_file, rp, to_realign, P)
    pr.disable(); t2 = time.time() - t
    rounds = len([f for f in os.listdir(tmp) if f.startswith("p_values_")])
    say("stat_filter_candidates: %.1f s, %d rounds -> %d final candidates (%d are true isoforms of %d)" % (t2, rounds, len(C), len(set(C.values()) & set(isoforms)), len(isoforms)), flush=True)
    say("whole pipeline: %.1f s for %d reads x ~%d bp" % (t1 + t2, n, L))
    # (the table bytes: the most the cached sets held when a round returned -- stat_filter_candidates frees them at its end)
    print("rank %d: stat_filter_candidates %.1f s, hypothesis tests shared between the ranks (none in a single process or under ISOCON_DEBUG_VARIANT=stat_all_edges): %s, "
          "rows uploaded %d, device table bytes %d" % (rank, t2, H.SHARD_STATS, H.DEVICE_STATS["rows_uploaded"], TABLE_BYTES[0]), flush=True)
    say("device read tables: %s" % H.DEVICE_STATS)
    say("edge variants on the device (isocon_edge_variants; none under ISOCON_DEBUG_VARIANT=stat_host_variants): %s" % H.EDGE_VARIANT_STATS, flush=True)
    say("bounds on the device (isocon_raghavan_bound; none under ISOCON_DEBUG_VARIANT=stat_host_bound): %s" % H.BOUND_STATS, flush=True)
    results = sorted(f for f in os.listdir(tmp) if f in ("final_candidates.fa", "cluster_info.tsv") or f.startswith("p_values_"))
    for f in results:          # the result files: their digests, and copies under $ISOCON_KEEP_RESULTS for a cmp between runs
        with open(os.path.join(tmp, f), "rb") as fh:
            print("%ssha256 %s %s" % ("rank %d: " % rank if dist is not None else "", hashlib.sha256(fh.read()).hexdigest(), f), flush=True)
        if os.environ.get("ISOCON_KEEP_RESULTS") and rank == 0:
            os.makedirs(os.environ["ISOCON_KEEP_RESULTS"], exist_ok=True)
            shutil.copy(os.path.join(tmp, f), os.environ["ISOCON_KEEP_RESULTS"])
    if rank == 0:
        pstats.Stats(pr).sort_stats("cumulative").print_stats(28)
if dist is not None:
    dist.barrier()
    dist.destroy_process_group()
