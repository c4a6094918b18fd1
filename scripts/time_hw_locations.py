"""SeqStore.hw_locations (isocon_hw_locations: every best location of an infix pair) against SeqStore.hw_pairs (one location, plus the
terminal insertion runs) on the same pair lists in one process, interleaved, three runs each: kernel and wall time, locations per
pair and the tiles per class of the ENDS and START launches.  Two lists:
  graph    the candidate-graph pair list of the synthetic C3 candidates (scripts/time_hw_graph.py: ~4 900 candidates of 10 isoforms,
           every candidate against its length window, k = 25) -- almost every hit has one end or a few adjacent ones
  repeats  short queries against targets that hold about 20 copies of them (primer / repeat searches)
--only-pairs: hw_pairs alone -- the form that runs on a tree without hw_locations (the parent commit's, for the comparison the
result file records).  Appends to --out (default profiles/hw_locations.txt).
Usage: python scripts/time_hw_locations.py [--only-pairs] [--label TEXT] [--out FILE] [--per N]"""
import argparse, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from isocon_amd import synth, end_invariant_functions as END
from isocon_amd import store as STORE
from isocon_amd.store import SeqStore

ap = argparse.ArgumentParser()
ap.add_argument("--only-pairs", action="store_true")
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hw_locations.txt"))
ap.add_argument("--per", type=int, default=490, help="candidates per isoform of the graph list")
args = ap.parse_args()
out = open(args.out, "a")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def graph_list():
    rng = np.random.Generator(np.random.PCG64(77))
    isoforms = synth.make_isoforms(rng, 2500, 10)
    prof = dict(rate=0.0012, ins=0.4, dele=0.4, sub=0.2)            # ~3 residual errors per candidate
    seqs = set()
    for iso in isoforms:
        for _ in range(args.per):
            s = synth.mutate(rng, iso, prof)
            a, b = int(rng.integers(0, 12)), int(rng.integers(0, 12))
            seqs.add(s[a:len(s) - b].tobytes().decode())
    seqs = sorted(seqs, key=len)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
    q, t = END._window_pairs(lens, 0, len(seqs), 40, 2 ** 32)
    return seqs, q, t, np.full(len(q), 25, dtype=np.int32)


def repeat_list(n_queries=500, per_query=64, copies=20):
    rng = random.Random(78)
    seqs, q, t = [], [], []
    for _ in range(n_queries):
        query = "".join(rng.choice("ACG") for _ in range(12))
        qi = len(seqs)
        seqs.append(query)
        for _ in range(per_query):
            c = list(query)
            for _ in range(rng.choice((0, 1, 2))):
                c[rng.randrange(2, 10)] = "T"
            c = "".join(c)
            q.append(qi)
            t.append(len(seqs))
            seqs.append("".join("T" * rng.randint(2, 6) + c for _ in range(copies)))
    return seqs, np.asarray(q, dtype=np.uint32), np.asarray(t, dtype=np.uint32), np.full(len(q), 2, dtype=np.int32)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, time.perf_counter() - t0


say("== %s (%s)" % (args.label, "hw_pairs alone" if args.only_pairs else "hw_locations against hw_pairs, interleaved"))
for name, (seqs, q, t, k) in (("graph", graph_list()), ("repeats", repeat_list())):
    st = SeqStore(seqs)
    st.hw_pairs(q[:4096], t[:4096], k[:4096])
    if not args.only_pairs:
        st.hw_locations(q[:4096], t[:4096], k[:4096])
    say("%s: %d sequences, %d pairs" % (name, len(seqs), len(q)))
    for rep in range(3):
        (rows, ms), wall = timed(lambda: st.hw_pairs(q, t, k, return_ms=True))
        say("  run %d  hw_pairs      kernels %8.2f ms  wall %7.3f s  hits %d" % (rep, ms, wall, int((rows[:, 0] >= 0).sum())))
        if args.only_pairs:
            continue
        (ed, ptr, locs, ms), wall = timed(lambda: st.hw_locations(q, t, k, return_ms=True))
        stats = STORE.hw_locations_last_stats()
        n = ptr.astype(np.int64)
        first = locs[n[:-1][ed >= 0]]
        same = bool((ed == rows[:, 0]).all() and (first == rows[ed >= 0][:, 1:3]).all())
        say("  run %d  hw_locations  kernels %8.2f ms  wall %7.3f s  hits %d  locations %d (%.2f per hit, most %d)  first location = hw_pairs: %s"
            % (rep, ms, wall, stats["hits"], stats["locations"], stats["locations"] / max(1, stats["hits"]), int(np.diff(n).max()), same))
    if not args.only_pairs:
        say("  tiles per class (1, 2, 4, 8 words): LOCATE %s  ENDS %s  START %s  host cuts %d"
            % tuple([[stats["%s_tiles_w%d" % (s, w)] for w in (1, 2, 4, 8)] for s in ("locate", "ends", "starts")] + [stats["host_cuts"]]))
    st.close()
