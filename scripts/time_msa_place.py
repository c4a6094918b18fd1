"""Wall time of the candidate phase (find_candidate_transcripts) and of its correction steps with the wide-slot insertions placed on the
device (the default) against the host route (ISOCON_DEBUG_VARIANT=msa_host_place), interleaved in one process: one warm-up run per route,
then `reps` runs per route; per run the summed and per-step wall time of _correct_all_from_ops, the HIP-event time of the builds' kernels,
the wide-slot records and the bytes of records and patches that cross the bus; medians at the end; asserts that both routes write the same
candidates.  profiles/msa_place.txt holds its output.  usage: time_msa_place.py c3|ont [n_reads] [reps]"""
import hashlib, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from isocon_amd import synth
from isocon_amd import isocon_get_candidates as IGC
from isocon_amd import correction_module as COR
from isocon_amd.store import SeqStore

which = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
if which == "c3":
    accs, seqs, isoforms = synth.make_reads(n, 2500, 10, 30001)
else:
    accs, seqs, isoforms = synth.make_reads(n, 0, 10, 50001, profile=dict(synth.ONT_PROFILE, rate=0.06), families=2, length_range=(1000, 2500))

acc = None
orig_all = COR._correct_all_from_ops
def timed_all(batch, *a):
    t0 = time.perf_counter(); out = orig_all(batch, *a); acc["step_s"].append(time.perf_counter() - t0); acc["kms"].append(getattr(batch.store, "msa_build_ms", float("nan"))); return out
COR._correct_all_from_ops = timed_all
orig_b, orig_pb, orig_c = SeqStore.msa_build_ops_batch, SeqStore.msa_build_ops_placed_batch, SeqStore.msa_correct_built_batch
def b(self, *a):
    out = orig_b(self, *a); acc["down"] += out[4].nbytes; acc["records"] += len(out[4]); return out
def pb(self, *a):
    out = orig_pb(self, *a); acc["down"] += out[4].nbytes; acc["records"] += len(out[4]) + out[5]; return out
def c(self, n_parts, n_rows, degree, packed_cap, patch_row=None, patch_col=None, patch_ptr=None, patch_bytes=None):
    if patch_row is not None:
        acc["up"] += 4 * len(patch_row) * 2 + 4 * len(patch_ptr) + len(patch_bytes)
    return orig_c(self, n_parts, n_rows, degree, packed_cap, patch_row, patch_col, patch_ptr, patch_bytes)
SeqStore.msa_build_ops_batch, SeqStore.msa_build_ops_placed_batch, SeqStore.msa_correct_built_batch = b, pb, c

with tempfile.TemporaryDirectory() as tmp:
    rf = os.path.join(tmp, "reads.fa")
    with open(rf, "w") as fh:
        for a_, s_ in zip(accs, seqs): fh.write(">%s\n%s\n" % (a_, s_))
    class P: nr_cores = 1; neighbor_search_depth = 2 ** 32; verbose = False; develop_logfile = None; logfile = None; min_exon_diff = 20
    P.ignore_ends_len = 15; P.min_candidate_support = 2; P.is_fastq = False; P.ccs = None

    def run(route, k):
        global acc
        acc = {"step_s": [], "kms": [], "down": 0, "up": 0, "records": 0}
        if route == "host": os.environ["ISOCON_DEBUG_VARIANT"] = "msa_host_place"
        else: os.environ.pop("ISOCON_DEBUG_VARIANT", None)
        P.outfolder = os.path.join(tmp, "%s%d" % (route, k)); os.makedirs(P.outfolder, exist_ok=True)
        before = dict(COR.PLACE_STATS)
        t = time.perf_counter(); cand_file, rp, to_realign = IGC.find_candidate_transcripts(rf, P); dt = time.perf_counter() - t
        digest = hashlib.sha1(open(cand_file, "rb").read()).hexdigest()[:12]
        st = {k_: COR.PLACE_STATS[k_] - before[k_] for k_ in before}
        print("%s %-6s run %d: pipeline %.3f s, %d correction steps, sum %.1f ms (per step median %.2f ms), build kernels sum %.2f ms, records %d, down %d B, up %d B, placed %d left %d, candidates %s" %
              (which, route, k, dt, len(acc["step_s"]), 1e3 * sum(acc["step_s"]), 1e3 * statistics.median(acc["step_s"]), sum(acc["kms"]), acc["records"], acc["down"], acc["up"],
               st["placed"], st["left"], digest), flush=True)
        return dt, 1e3 * sum(acc["step_s"]), sum(acc["kms"]), digest, [1e3 * x for x in acc["step_s"]], list(acc["kms"])

    res = {"device": [], "host": []}
    for route in ("device", "host"):
        run(route, -1)          # warm-up
    for k in range(reps):
        for route in (("device", "host") if k % 2 == 0 else ("host", "device")):
            res[route].append(run(route, k))
    for route in ("device", "host"):
        r = res[route]
        print("%s %-6s median of %d: pipeline %.3f s [%.3f .. %.3f], correction steps %.1f ms [%.1f .. %.1f], build kernels %.2f ms" %
              (which, route, len(r), statistics.median(x[0] for x in r), min(x[0] for x in r), max(x[0] for x in r), statistics.median(x[1] for x in r), min(x[1] for x in r),
               max(x[1] for x in r), statistics.median(x[2] for x in r)), flush=True)
    for route in ("device", "host"):
        steps = np.median(np.array([x[4] for x in res[route]]), axis=0); kms = np.median(np.array([x[5] for x in res[route]]), axis=0)
        print("%s %-6s per step (median over runs) wall ms: %s" % (which, route, " ".join("%.1f" % x for x in steps)))
        print("%s %-6s per step (median over runs) build kernel ms: %s" % (which, route, " ".join("%.2f" % x for x in kms)))
    assert len({x[3] for r in res.values() for x in r}) == 1, "the routes disagree"
    print("%s: both routes give the same candidates" % which)
