"""Infix alignments of the candidate-vs-candidate graph (end_invariant_functions.get_all_NN) at ignore_ends_len = 15 -- the banded
kernels, the path every default run takes -- and at ignore_ends_len = 150, where pairs whose band exceeds 512 diagonals go through the
un-banded kernels of csrc/hw_full.hpp (SeqStore.hw_pairs(wide=True) = isocon_hw_pairs_wide).  Seeded stand-in of the C3 candidate set:
10 isoforms x `per` candidates of about `length` bases with ~3 residual errors, ends cut by 0 .. `ends` bases.  Median of 5 calls after
a warm-up; the CPU oracle's time for a 1 000-pair sample stands beside the new path.  Appends to profiles/hw_wide.txt.
Usage: python scripts/time_hw_wide.py [--per 490] [--length 2500] [--ends 12] [--ignore 15,150] [--label text] [--out file]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from isocon_amd import synth, end_invariant_functions as END
from isocon_amd.store import SeqStore

ap = argparse.ArgumentParser()
ap.add_argument("--per", type=int, default=490)
ap.add_argument("--length", type=int, default=2500)
ap.add_argument("--ends", type=int, default=12)
ap.add_argument("--ignore", default="15,150")
ap.add_argument("--label", default="")
ap.add_argument("--oracle-sample", type=int, default=1000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hw_wide.txt"))
args = ap.parse_args()

rng = np.random.Generator(np.random.PCG64(77))
isoforms = synth.make_isoforms(rng, args.length, 10)
prof = dict(rate=0.0012, ins=0.4, dele=0.4, sub=0.2)
seqs = set()
for iso in isoforms:
    for _ in range(args.per):
        s = synth.mutate(rng, iso, prof)
        a, b = int(rng.integers(0, args.ends + 1)), int(rng.integers(0, args.ends + 1))
        seqs.add(s[a:len(s) - b].tobytes().decode())
seqs = sorted(seqs, key=len)
lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
st = SeqStore(seqs)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say("# %s%d candidates of %d .. %d bases (per %d, length %d, ends 0 .. %d)" % (args.label + ": " if args.label else "", len(seqs), lens[0], lens[-1], args.per, args.length, args.ends))
for ig in [int(x) for x in args.ignore.split(",")]:
    kk, window = 10 + ig, 10 + 2 * ig
    wide = window + 2 * kk + 1 > 512                       # the rule of get_all_NN
    q, t = END._window_pairs(lens, 0, len(seqs), window, 2 ** 32)
    k = np.full(len(q), kk, dtype=np.int32)
    kw = dict(wide=True) if wide else {}
    n_wide = int((np.maximum(lens[t] - lens[q], 0) + 2 * kk + 1 > 512).sum())
    st.hw_pairs(q[:4096], t[:4096], k[:4096], **kw)        # warm-up
    walls, kms = [], []
    for rep in range(5):
        t0 = time.perf_counter()
        res, ms = st.hw_pairs(q, t, k, return_ms=True, **kw)
        walls.append(time.perf_counter() - t0)
        kms.append(ms)
    say("ignore_ends_len %3d (k %d, window %d, %s): %d pairs, %d beyond 512 diagonals, %d hits: wall median %.1f ms (min %.1f, max %.1f), kernels median %.1f ms"
        % (ig, kk, window, "isocon_hw_pairs_wide" if wide else "isocon_hw_pairs", len(q), n_wide, int((res[:, 0] >= 0).sum()),
           1e3 * float(np.median(walls)), 1e3 * min(walls), 1e3 * max(walls), float(np.median(kms))))
    if wide and args.oracle_sample:
        from oracle import oracle as O
        pick = np.random.Generator(np.random.PCG64(5)).choice(len(q), size=min(args.oracle_sample, len(q)), replace=False)
        t0 = time.perf_counter()
        bad = 0
        for p in pick.tolist():
            ed, start, end = O.hw_locate(seqs[q[p]], seqs[t[p]], kk)
            row = [-1, -1, -1, 0, 0]
            if ed >= 0:
                _, ops = O.nw_path(seqs[q[p]], seqs[t[p]][start:end + 1])
                row = [ed, start, end, ops[0][0] if ops[0][1] == "I" else 0, ops[-1][0] if ops[-1][1] == "I" else 0]
            bad += row != res[p].tolist()
        say("    CPU oracle (full matrices, one core), the same call's sample of %d pairs: %.2f s; rows that differ from the GPU's: %d" % (len(pick), time.perf_counter() - t0, bad))
st.close()
with open(args.out, "a") as f:
    f.write("\n".join(lines) + "\n")
