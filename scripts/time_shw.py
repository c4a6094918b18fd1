"""SeqStore.shw_locations (isocon_shw_locations: prefix alignments of a pair list) on the synthetic C3 reads, warm, three runs each: kernel
milliseconds, the call's wall time and the pairs entering each round.  Three lists:
  primer k=5      the first 30 bases of an isoform (one 30-base query) against every read, k = 5
  primer k=None   the same, unbounded
  reads k=100     50 000 read x read pairs (a read against the read --stride places behind it), k = 100
For scale only, every line also carries the CPU restatement (the last row of the global matrix, a numpy row at a time -- min over j of
oracle.ed_dp(q, t[:j]) in one pass, checked against it on the first sampled pair of the primer lists -- on --sample pairs, the target cut
to len(q) + k columns as the definition allows) extrapolated to the list.  No device route exists at the parent commit to compare with.
Appends to --out (default profiles/shw.txt).
Usage: python scripts/time_shw.py [--reads N] [--sample N] [--label TEXT] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from isocon_amd import synth
from isocon_amd import store as STORE
from isocon_amd.store import SeqStore
from oracle import oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=50000)
ap.add_argument("--sample", type=int, default=20)
ap.add_argument("--stride", type=int, default=7)
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shw.txt"))
args = ap.parse_args()
out = open(args.out, "a")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


def prefix_distance(x, y):
    """min over j >= 1 of D[len(x)][j], D the global matrix (row 0 = j)"""
    tt = np.frombuffer(y.encode(), dtype=np.uint8)
    ar = np.arange(len(y) + 1, dtype=np.int64)
    prev = ar.copy()
    for i, c in enumerate(x.encode(), 1):
        cur = np.empty(len(y) + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (tt != c))
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[1:].min())


def cpu_seconds(seqs, q, t, k):
    """the restatement on a sample of the list, extrapolated to all of it"""
    idx = np.linspace(0, len(q) - 1, min(args.sample, len(q))).astype(np.int64)
    t0 = time.perf_counter()
    for p in idx:
        x, y = seqs[q[p]], seqs[t[p]]
        prefix_distance(x, y[:len(x) + (len(x) if k is None else k)])
    dt = time.perf_counter() - t0
    x, y = seqs[q[idx[0]]], seqs[t[idx[0]]][:2 * len(seqs[q[idx[0]]])]
    if len(x) <= 64:
        assert prefix_distance(x, y) == min(O.ed_dp(x, y[:j]) for j in range(1, len(y) + 1))
    return dt / len(idx) * len(q)


accs, reads, isoforms = synth.make_reads(args.reads, 2500, 10, 30001)
seqs = list(reads) + [isoforms[0][:30]]
n = len(reads)
primer = np.full(n, n, dtype=np.uint32)
every = np.arange(n, dtype=np.uint32)
lists = (("primer k=5", primer, every, 5), ("primer k=None", primer, every, None),
         ("reads k=100", every, (every + args.stride) % n, 100))
st = SeqStore(seqs)
say("== %s: %d reads (C3 synthetic, seed 30001), one 30-base query" % (args.label, n))
for name, q, t, k in lists:
    st.shw_locations(q[:4096], t[:4096], k)          # warm
    cpu = cpu_seconds(seqs, q, t, k)
    for rep in range(3):
        (ed, ptr, ends, ms), wall = timed(lambda: st.shw_locations(q, t, k, return_ms=True))
        s = STORE.shw_last_stats()
        say("  %-14s run %d  %d pairs  kernels %8.2f ms  wall %7.3f s  hits %d  ends %d  rounds %d  entering %s  LOCATE tiles %s  ENDS tiles %s  (CPU restatement, extrapolated from %d pairs: %.1f s)"
            % (name, rep, len(q), ms, wall, s["hits"], s["ends"], s["rounds"], [s["enter_round%d" % r] for r in range(4)],
               [s["locate_tiles_w%d" % w] for w in (1, 2, 4, 8)], [s["ends_tiles_w%d" % w] for w in (1, 2, 4, 8)], min(args.sample, len(q)), cpu))
st.close()
