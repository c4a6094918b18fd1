"""Global alignment paths of a pair list on the device (SeqStore.ed_path_pairs = isocon_ed_path_pairs, csrc/nw_path.hpp): `pairs`
related pairs of reads of about `length` bases (two reads of one isoform with i.i.d. errors each: distances of about 20-60).  Median
of 5 calls after a warm-up: wall and kernel ms, the route the hits took (store.path_last_stats: classes of the banded kernels, bytes of
trace, launches, kernel ms; ISOCON_DEBUG_VARIANT=nwp_unbanded times the un-banded kernel), what the un-banded store would be, and its
overhead (64-row blocks computed and stored per column against those a trace restricted to the diagonals within ed of the
corner-to-corner corridor would need).  Beside it: oracle.nw_path (full matrix in C, one core) on a sample of the same list, paths
compared, and on 3 pairs the host route edlib_traceback took before the device route existed (the distance from isocon_ed_pairs, then
functions.nw_path_cigar: a full matrix of Python ints).  Appends to profiles/ed_path.txt.
Usage: python scripts/time_ed_path.py [--pairs 2000] [--length 2500] [--rate 0.008] [--oracle-sample 50] [--host-sample 3] [--label text] [--out file]"""
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
ap.add_argument("--oracle-sample", type=int, default=50)
ap.add_argument("--host-sample", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed_path.txt"))
args = ap.parse_args()

rng = np.random.Generator(np.random.PCG64(91))
isoforms = synth.make_isoforms(rng, args.length, 10)
prof = dict(rate=args.rate, ins=0.4, dele=0.4, sub=0.2)
seqs = []
for p in range(args.pairs):
    iso = isoforms[p % len(isoforms)]
    seqs += [synth.mutate(rng, iso, prof).tobytes().decode(), synth.mutate(rng, iso, prof).tobytes().decode()]
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


st.ed_path_pairs(q[:64], t[:64])          # warm-up
walls, kms = [], []
for rep in range(5):
    t0 = time.perf_counter()
    ed, ops, ops_ptr, ms = st.ed_path_pairs(q, t, return_ms=True)
    walls.append(time.perf_counter() - t0)
    kms.append(ms)
stats = path_last_stats()
need = np.array([trace_bytes(int(lens[a]), int(lens[b])) for a, b in zip(q, t)], dtype=np.int64)
launches, held = 1, 0
for b in need.tolist():          # the host's cut (nwp_plan.hpp): consecutive pairs while their stores fit 1 GiB together
    if held + b > (1 << 30):
        launches, held = launches + 1, 0
    held += b
m, n = lens[q], lens[t]
blocks_full = (m + 63) // 64
blocks_band = np.minimum(blocks_full, (2 * ed + 1 + np.abs(n - m) + 63) // 64 + 1)
say("# %s%d pairs of %d .. %d bases (length %d, error rate %.4f per read), distances %d .. %d (median %d), %d ops (%.1f per pair)"
    % (args.label + ": " if args.label else "", args.pairs, lens.min(), lens.max(), args.length, args.rate, ed.min(), ed.max(), int(np.median(ed)), len(ops), len(ops) / args.pairs))
say("ed_path_pairs: wall median %.1f ms (min %.1f, max %.1f), kernels median %.1f ms; the un-banded trace would be %.2f MB per pair (%.2f GB in all), %d launches under the 1 GiB budget"
    % (1e3 * float(np.median(walls)), 1e3 * min(walls), 1e3 * max(walls), float(np.median(kms)), need.mean() / 1e6, need.sum() / 1e9, launches))
say("    route of the hits (store.path_last_stats; ISOCON_DEBUG_VARIANT=%s): W = 1 / 2 / 4: %d / %d / %d, un-banded %d; trace %.3f MB banded + %.3f MB un-banded; launches %d + %d; "
    "kernels of the last call: banded trace + walk %.2f ms, un-banded %.2f ms, forward ops %.2f ms"
    % (os.environ.get("ISOCON_DEBUG_VARIANT", ""), stats["hits_w1"], stats["hits_w2"], stats["hits_w4"], stats["hits_unbanded"], stats["trace_bytes_band"] / 1e6,
       stats["trace_bytes_unbanded"] / 1e6, stats["launches_band"], stats["launches_unbanded"], stats["band_ms"], stats["unbanded_ms"], stats["emit_ms"]))
say("    un-banded overhead: %.1f blocks of 64 rows per column computed and stored, %.1f would hold the diagonals within ed of the corridor: factor %.1f"
    % (blocks_full.mean(), blocks_band.mean(), float((blocks_full / blocks_band).mean())))
if args.oracle_sample:
    from oracle import oracle as O
    pick = np.random.Generator(np.random.PCG64(5)).choice(args.pairs, size=min(args.oracle_sample, args.pairs), replace=False)
    t0 = time.perf_counter()
    bad = 0
    for p in pick.tolist():
        e, path = O.nw_path(seqs[q[p]], seqs[t[p]])
        got = [(int(o) >> 4, "=XID"[int(o) & 15]) for o in ops[int(ops_ptr[p]):int(ops_ptr[p + 1])]]
        bad += (e, path) != (int(ed[p]), got)
    say("    CPU oracle (full matrix, one core), a sample of %d pairs of the list: %.2f s; paths that differ from the GPU's: %d" % (len(pick), time.perf_counter() - t0, bad))
if args.host_sample:
    from isocon_amd.edlib_alignment_module import _cigar_of_steps
    from isocon_amd.functions import nw_path_cigar
    t0 = time.perf_counter()
    bad = 0
    for p in range(args.host_sample):
        x, y = seqs[q[p]], seqs[t[p]]
        one = SeqStore([x, y])
        e = int(one.ed_pairs([0], [1], None)[0])
        one.close()
        cigar = _cigar_of_steps(nw_path_cigar(x, y))
        bad += (e, cigar) != (int(ed[p]), "".join("%d%s" % (int(o) >> 4, "=XID"[int(o) & 15]) for o in ops[int(ops_ptr[p]):int(ops_ptr[p + 1])]))
    dt = time.perf_counter() - t0
    say("    host route of edlib_traceback before this entry point (distance on the GPU, path by functions.nw_path_cigar), %d pairs: %.2f s (%.2f s per pair); results that differ: %d"
        % (args.host_sample, dt, dt / args.host_sample, bad))
st.close()
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
