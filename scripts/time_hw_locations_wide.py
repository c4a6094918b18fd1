"""SeqStore.hw_locations(wide=True) (isocon_hw_locations_wide: every best location of an infix pair, bands above 512 diagonals too)
against SeqStore.hw_pairs(wide=True) (one location per pair: the only answer a tree without the entry has for these pairs) on the same
pair lists in one process, interleaved, three runs each after a warm-up: kernel and wall time, hits, locations per hit, routes.
  primers  the synthetic C3 reads (isocon_amd/synth.py: 50 000 reads of ~2.5 kb) against a handful of 20- to 40-base queries cut from
           them, k = 3
  rows<N>  queries of N = 65, 128, 129, 256 bases cut from the reads against --route-reads of them, k = 3, once per route of the
           wide part (ISOCON_DEBUG_VARIANT=hwl_rows_max=<rows>: one lane per pair with N <= rows, one wavefront per pair otherwise)
--only-pairs: hw_pairs(wide=True) alone -- the form that runs on a tree without the entry (the parent commit's, for the comparison the
result file records).  Appends to --out (default profiles/hw_locations_wide.txt).
Usage: python scripts/time_hw_locations_wide.py [--only-pairs] [--label TEXT] [--out FILE] [--reads N] [--queries N] [--route-reads N]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from isocon_amd import synth
from isocon_amd.store import SeqStore

ap = argparse.ArgumentParser()
ap.add_argument("--only-pairs", action="store_true")
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hw_locations_wide.txt"))
ap.add_argument("--reads", type=int, default=50000)
ap.add_argument("--queries", type=int, default=6)
ap.add_argument("--route-reads", type=int, default=20000)
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


def with_variant(value, f):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    if value:
        os.environ["ISOCON_DEBUG_VARIANT"] = (saved + "," if saved else "") + value
    try:
        return f()
    finally:
        if value:
            if saved is None:
                del os.environ["ISOCON_DEBUG_VARIANT"]
            else:
                os.environ["ISOCON_DEBUG_VARIANT"] = saved


def spread(v):
    return "median %.2f (min %.2f, max %.2f)" % (float(np.median(v)), min(v), max(v))


accs, reads, isoforms = synth.make_reads(args.reads, 2500, 10, 30001)
reads = sorted(set(reads))
rng = np.random.Generator(np.random.PCG64(79))


def cut(length):
    r = reads[int(rng.integers(0, len(reads)))]
    at = int(rng.integers(0, len(r) - length))
    return r[at:at + length]


def pair_list(queries, n_reads):
    """every query against the first n_reads reads: (seqs, q, t, k)"""
    seqs = reads[:n_reads] + list(queries)
    q = np.repeat(np.arange(n_reads, n_reads + len(queries), dtype=np.uint32), n_reads)
    t = np.tile(np.arange(n_reads, dtype=np.uint32), len(queries))
    return seqs, q, t, np.full(len(q), 3, dtype=np.int32)


def measure(name, seqs, q, t, k, variants):
    st = SeqStore(seqs)
    say("%s: %d sequences, %d pairs" % (name, len(seqs), len(q)))
    st.hw_pairs(q[:4096], t[:4096], k[:4096], wide=True)
    if not args.only_pairs:
        for v in variants:
            with_variant(v, lambda: st.hw_locations(q[:4096], t[:4096], k[:4096], wide=True))
    pairs_ms, loc_ms = [], {v: [] for v in variants}
    for rep in range(3):
        (rows, ms), wall = timed(lambda: st.hw_pairs(q, t, k, return_ms=True, wide=True))
        pairs_ms.append(ms)
        say("  run %d  hw_pairs(wide)                    kernels %9.2f ms  wall %7.3f s  hits %d" % (rep, ms, wall, int((rows[:, 0] >= 0).sum())))
        if args.only_pairs:
            continue
        for v in variants:
            (ed, ptr, locs, ms), wall = with_variant(v, lambda: timed(lambda: st.hw_locations(q, t, k, return_ms=True, wide=True)))
            stats = st.hw_locations_wide_last_stats()
            loc_ms[v].append(ms)
            n = ptr.astype(np.int64)
            first = locs[n[:-1][ed >= 0]]
            same = bool((ed == rows[:, 0]).all() and (first == rows[ed >= 0][:, 1:3]).all())
            say("  run %d  hw_locations(wide) %-14s kernels %9.2f ms  wall %7.3f s  hits %d  locations %d (%.2f per hit)  lanes w1/w2/w4 %d/%d/%d  wavefront %d  "
                "starts banded/un-banded %d/%d  launches %d  first location = hw_pairs: %s"
                % (rep, v or "(default)", ms, wall, stats["hits"], stats["locations"], stats["locations"] / max(1, stats["hits"]), stats["rows_w1"], stats["rows_w2"],
                   stats["rows_w4"], stats["wave"], stats["starts_banded"], stats["starts_unbanded"], stats["launches"], same))
    say("  hw_pairs(wide) kernel ms: %s" % spread(pairs_ms))
    for v in variants:
        if loc_ms[v]:
            say("  hw_locations(wide) %s kernel ms: %s; hw_pairs(wide) / hw_locations(wide) of the medians: %.2f"
                % (v or "(default)", spread(loc_ms[v]), float(np.median(pairs_ms)) / max(1e-9, float(np.median(loc_ms[v])))))
    st.close()


say("== %s (%s)" % (args.label, "hw_pairs(wide=True) alone" if args.only_pairs else "hw_locations(wide=True) against hw_pairs(wide=True), interleaved"))
lengths = [20, 24, 28, 32, 36, 40, 22, 30, 34, 38][:args.queries]
measure("primers", *pair_list([cut(n) for n in lengths], len(reads)), variants=[""])
for rows in (65, 128, 129, 256):
    measure("rows%d" % rows, *pair_list([cut(rows)], min(args.route_reads, len(reads))), variants=["hwl_rows_max=256", "hwl_rows_max=64"])
