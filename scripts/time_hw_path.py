"""Infix alignment paths of a pair list on the device (SeqStore.hw_path_pairs = isocon_hw_path_pairs, the windowed instance of
csrc/nw_path.hpp): the `pairs` related pairs of scripts/time_ed_path.py (two reads of one isoform with i.i.d. errors each), the query
being the first read with 20-100 bases trimmed from either end, the target the second read.  Median of 5 calls after a warm-up: wall
and kernel ms under a threshold the banded locate takes (--k) and unbounded (the un-banded locate), number of ops and bytes of trace.
Beside them, on the same pairs in the same session, what the path costs on top of the location: hw_pairs(wide=True) alone, and
ed_path_pairs on (query, located window) -- the trace-and-walk alone, through the whole-target instance.  A sample of the paths is
compared with oracle.hw_path.  Appends to profiles/hw_path.txt.
Usage: python scripts/time_hw_path.py [--pairs 2000] [--length 2500] [--rate 0.008] [--k 100] [--oracle-sample 20] [--label text] [--out file]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from isocon_amd import synth
from isocon_amd.store import SeqStore, path_last_stats

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2000)
ap.add_argument("--length", type=int, default=2500)
ap.add_argument("--rate", type=float, default=0.008)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--oracle-sample", type=int, default=20)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hw_path.txt"))
args = ap.parse_args()

rng = np.random.Generator(np.random.PCG64(91))
isoforms = synth.make_isoforms(rng, args.length, 10)
prof = dict(rate=args.rate, ins=0.4, dele=0.4, sub=0.2)
seqs = []
for p in range(args.pairs):
    iso = isoforms[p % len(isoforms)]
    seqs += [synth.mutate(rng, iso, prof).tobytes().decode(), synth.mutate(rng, iso, prof).tobytes().decode()]
trim = np.random.Generator(np.random.PCG64(92)).integers(20, 101, size=(args.pairs, 2))
for p in range(args.pairs):
    seqs[2 * p] = seqs[2 * p][int(trim[p, 0]):len(seqs[2 * p]) - int(trim[p, 1])]
q = np.arange(0, 2 * args.pairs, 2, dtype=np.uint32)
t = q + 1
lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
st = SeqStore(seqs)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def trace_bytes(m, ms):
    """hwf_trace_units (csrc/hw_full_core.hpp) x 16"""
    blocks = (m + 63) // 64
    last = (blocks + 63) // 64 - 1
    r32 = lambda u: (u + 31) & ~31
    lanes = blocks - 64 * last
    return 16 * (r32((blocks + 1) // 2) + last * r32((ms + 63) * 64) + r32((ms + lanes - 1) * lanes))


def median5(call):
    walls, kms, out = [], [], None
    for rep in range(5):
        t0 = time.perf_counter()
        out = call()
        walls.append(time.perf_counter() - t0)
        kms.append(out[-1])
    return out, "wall median %.1f ms (min %.1f, max %.1f), kernels median %.1f ms" % (1e3 * float(np.median(walls)), 1e3 * min(walls), 1e3 * max(walls), float(np.median(kms)))


st.hw_path_pairs(q[:64], t[:64], args.k)          # warm-up
st.hw_path_pairs(q[:64], t[:64])
st.ed_path_pairs(q[:64], t[:64])
(rows, ops, ops_ptr, _), path_k = median5(lambda: st.hw_path_pairs(q, t, args.k, return_ms=True))
stats_k = path_last_stats()
(rows_u, ops_u, ops_ptr_u, _), path_u = median5(lambda: st.hw_path_pairs(q, t, return_ms=True))
(loc, _), loc_k = median5(lambda: st.hw_pairs(q, t, args.k, return_ms=True, wide=True))
(loc_u, _), loc_un = median5(lambda: st.hw_pairs(q, t, lens[q].astype(np.int32), return_ms=True, wide=True))
hit = rows[:, 0] >= 0
cols = (rows[:, 2] - rows[:, 1] + 1)[hit]
need = np.array([trace_bytes(int(m), int(c)) for m, c in zip(lens[q][hit], cols)], dtype=np.int64)
whole = np.array([trace_bytes(int(m), int(n)) for m, n in zip(lens[q][hit], lens[t][hit])], dtype=np.int64)
say("# %s%d pairs: queries of %d .. %d bases inside targets of %d .. %d (length %d, error rate %.4f per read, 20-100 bases trimmed from either end of the query)"
    % (args.label + ": " if args.label else "", args.pairs, lens[q].min(), lens[q].max(), lens[t].min(), lens[t].max(), args.length, args.rate))
say("hw_path_pairs, k = %d (%d hits, distances %d .. %d, median %d): %s; %d ops (%.1f per hit); the un-banded trace would be %.2f MB per hit (%.2f GB in all; the whole target %.2f GB)"
    % (args.k, int(hit.sum()), rows[hit, 0].min() if hit.any() else -1, rows[hit, 0].max() if hit.any() else -1, int(np.median(rows[hit, 0])) if hit.any() else -1, path_k,
       len(ops), len(ops) / max(int(hit.sum()), 1), need.mean() / 1e6 if hit.any() else 0.0, need.sum() / 1e9, whole.sum() / 1e9))
say("    route of the hits (store.path_last_stats; ISOCON_DEBUG_VARIANT=%s): W = 1 / 2 / 4: %d / %d / %d, un-banded %d; trace %.3f MB banded + %.3f MB un-banded; launches %d + %d; "
    "kernels of the last call: banded trace + walk %.2f ms, un-banded %.2f ms, forward ops %.2f ms"
    % (os.environ.get("ISOCON_DEBUG_VARIANT", ""), stats_k["hits_w1"], stats_k["hits_w2"], stats_k["hits_w4"], stats_k["hits_unbanded"], stats_k["trace_bytes_band"] / 1e6,
       stats_k["trace_bytes_unbanded"] / 1e6, stats_k["launches_band"], stats_k["launches_unbanded"], stats_k["band_ms"], stats_k["unbanded_ms"], stats_k["emit_ms"]))
say("    hw_pairs(wide=True) alone, k = %d: %s; rows equal: %s" % (args.k, loc_k, bool((loc == rows).all())))
say("hw_path_pairs, unbounded (k = len(q): the un-banded locate): %s; %d hits, %d ops; same paths as under k = %d for its hits: %s"
    % (path_u, int((rows_u[:, 0] >= 0).sum()), len(ops_u), args.k,
       all(ops_u[int(ops_ptr_u[p]):int(ops_ptr_u[p + 1])].tolist() == ops[int(ops_ptr[p]):int(ops_ptr[p + 1])].tolist() for p in np.flatnonzero(hit).tolist())))
say("    hw_pairs(wide=True) alone, k = len(q): %s; rows equal: %s" % (loc_un, bool((loc_u == rows_u).all())))
# the trace-and-walk alone: global paths of (query, located window) through the whole-target instance
hits = np.flatnonzero(rows_u[:, 0] >= 0)
wseqs = []
for p in hits.tolist():
    wseqs += [seqs[2 * p], seqs[2 * p + 1][int(rows_u[p, 1]):int(rows_u[p, 2]) + 1]]
ws = SeqStore(wseqs)
wq = np.arange(0, len(wseqs), 2, dtype=np.uint32)
ws.ed_path_pairs(wq[:64], wq[:64] + 1)
(ed_w, ops_w, ops_ptr_w, _), glob = median5(lambda: ws.ed_path_pairs(wq, wq + 1, rows_u[hits, 0], return_ms=True))
same = bool((ed_w == rows_u[hits, 0]).all()) and ops_w.tolist() == ops_u.tolist()
say("    ed_path_pairs on (query, window) of the %d hits, k = the distance: %s; same distances and ops: %s" % (len(hits), glob, same))
ws.close()
if args.oracle_sample:
    from oracle import oracle as O
    pick = np.random.Generator(np.random.PCG64(5)).choice(args.pairs, size=min(args.oracle_sample, args.pairs), replace=False)
    t0 = time.perf_counter()
    bad = 0
    for p in pick.tolist():
        e = O.hw_path(seqs[q[p]], seqs[t[p]], -1)
        got = "".join("%d%s" % (int(o) >> 4, "=XID"[int(o) & 15]) for o in ops_u[int(ops_ptr_u[p]):int(ops_ptr_u[p + 1])])
        bad += (e["editDistance"], e["locations"], e["cigar"]) != (int(rows_u[p, 0]), [(int(rows_u[p, 1]), int(rows_u[p, 2]))], got)
    say("    CPU oracle (hw_locate + full matrix of the window, one core), a sample of %d pairs of the list: %.2f s; results that differ from the GPU's: %d"
        % (len(pick), time.perf_counter() - t0, bad))
st.close()
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
