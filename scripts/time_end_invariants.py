"""Wall time of end_invariant_functions.collapse_candidates_under_ends_invariant by route: the device route (isocon_end_invariant_graph) and
the host route of the same build (ISOCON_DEBUG_VARIANT=inv_host_graph: the anchor index and the CPython helper, the code the function ran
before the device route existed), interleaved in one process, median of --runs timed runs after one warm-up run of each.  Two synthetic
candidate sets (isocon_amd/synth.py isoforms; a candidate = an isoform with a few substitutions and trimmed or extended ends):
  c3   about 1 000 candidates of about 2.5 kb in 10 isoforms
  c5   about 30 000 candidates of 1-5 kb in 50 isoforms (10 genes)
Prints, and with --out writes, one table per set: wall time per route, the kernel time and the four counters of the device call, and
whether the two partitions are equal.  --also FILE: a third leg, another version of end_invariant_functions.py (the parent commit's, say).
Needs a GPU: a measurement without one fails.  Usage: python scripts/time_end_invariants.py [--shapes c3,c5] [--runs 5] [--out FILE]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isocon_amd import end_invariant_functions as END  # noqa: E402
from isocon_amd import synth  # noqa: E402

SHAPES = {"c3": dict(count=1000, length=2500, n_isoforms=10, families=1, length_range=None, seed=301),
          "c5": dict(count=30000, length=3000, n_isoforms=50, families=10, length_range=(1000, 5000), seed=501)}
THR = 15          # (the product's default ignore_ends_len)


def candidates(count, length, n_isoforms, families, length_range, seed):
    """{acc: seq}, {acc: support}: every candidate is an isoform with 0 (one in ten) or 1-4 substitutions, its ends trimmed by up to 20 bases
    (half of them), extended by up to 20 random bases at one end (a quarter) or left alone"""
    _, _, isoforms = synth.make_reads(1, length, n_isoforms, seed, families=families, length_range=length_range)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    C, support, seen = {}, {}, set()
    for i in range(count):
        b = np.frombuffer(isoforms[i % len(isoforms)].encode(), dtype=np.uint8).copy()
        if rng.random() >= 0.1:
            pos = rng.choice(len(b), size=int(rng.integers(1, 5)), replace=False)
            b[pos] = acgt[(np.searchsorted(acgt, b[pos]) + rng.integers(1, 4, size=len(pos))) % 4]
        r = rng.random()
        if r < 0.5:
            b = b[int(rng.integers(0, 21)):len(b) - int(rng.integers(0, 21))]
        elif r < 0.75:
            ext = acgt[rng.integers(0, 4, size=int(rng.integers(0, 21)))]
            b = np.concatenate([ext, b]) if rng.random() < 0.5 else np.concatenate([b, ext])
        s = b.tobytes().decode("ascii")
        if s not in seen:
            seen.add(s)
            C["cand_%d" % i] = s
            support["cand_%d" % i] = 1 + i % 7
    return C, support


class Params(object):
    ignore_ends_len = THR
    verbose = False


def timed(fn, host):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    if host:
        os.environ["ISOCON_DEBUG_VARIANT"] = (saved + "," if saved else "") + "inv_host_graph"
    try:
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out          # (the device call ends with its downloads: nothing is left in flight)
    finally:
        if host:
            if saved is None:
                del os.environ["ISOCON_DEBUG_VARIANT"]
            else:
                os.environ["ISOCON_DEBUG_VARIANT"] = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--also")
    args = ap.parse_args()
    legs = [("device", END, False), ("host", END, True)]
    if args.also:
        spec = importlib.util.spec_from_file_location("isocon_amd._other_end_invariant_functions", args.also)
        other = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(other)
        legs.append(("also", other, True))
    lines = ["# collapse_candidates_under_ends_invariant, ignore_ends_len %d: wall time by route, median of %d runs after a warm-up, the routes interleaved in one process"
             % (THR, args.runs), "# (scripts/time_end_invariants.py; host = ISOCON_DEBUG_VARIANT=inv_host_graph, the anchor index and CPython helper)"]
    for shape in args.shapes.split(","):
        C, support = candidates(**SHAPES[shape])
        lens = [len(s) for s in C.values()]
        walls = {name: [] for name, _, _ in legs}
        results = {}
        kernel_ms, ctr = [], None
        for run in range(args.runs + 1):
            for name, mod, host in legs:
                before = dict(END.INVARIANT_STATS)
                wall, part = timed(lambda: mod.collapse_candidates_under_ends_invariant(C, support, Params()), host)
                ran_device = END.INVARIANT_STATS["device_calls"] - before["device_calls"]
                if (name == "device") != (ran_device == 1):
                    raise SystemExit("%s leg of %s: %d device calls" % (name, shape, ran_device))
                if run:
                    walls[name].append(wall)
                    if name == "device":
                        kernel_ms.append(END.INVARIANT_STATS["kernel_ms"] - before["kernel_ms"])
                results[name] = part
        rows, _, ctr = END._device_invariant_rows([s for _, s in sorted(C.items(), key=lambda x: len(x[1]))], THR)
        same = all(list(results[name].items()) == list(results["device"].items()) for name in results)
        lines.append("")
        lines.append("%s: %d candidates of %d-%d bases, %d kept after the collapse; partitions of all routes equal, order included: %s"
                     % (shape, len(C), min(lens), max(lens), len(results["device"]), same))
        for name, _, _ in legs:
            w = walls[name]
            lines.append("  %-7s wall  median %9.4f s   min %9.4f s   runs %s" % (name, statistics.median(w), min(w), " ".join("%.4f" % x for x in w)))
        lines.append("  device  kernels  median %.3f ms   runs %s" % (statistics.median(kernel_ms), " ".join("%.3f" % x for x in kernel_ms)))
        lines.append("  device  counters  window pairs %d   (pair, shift) survivors of the first-word test %d   pairs fully verified %d   invariant pairs %d"
                     % (ctr["pairs"], ctr["survivors"], ctr["verified"], ctr["invariant"]))
        print("\n".join(lines[-(4 + len(legs)):]), flush=True)
        if not same:
            raise SystemExit("the routes disagree on %s" % shape)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
