"""Wall and kernel time of the reads x candidates search with a neighbor_search_depth that binds, on a g19 set (tests/golden/make_golden_g19.py:
c2 = 5 000 reads, c3 = 50 000 reads against their seeded candidates) through the public compute_2set_nearest_neighbor_graph.

    python scripts/time_2set_depth.py c2 8            # one warm-up call, then the median of 5
    python scripts/time_2set_depth.py c3 16 256       # several depths on one set
    python scripts/time_2set_depth.py --variant nn2_probe_stride=4 c3 256          # ISOCON_DEBUG_VARIANT for the run: the block test's
                                                      # other probe stride, nn_no_block_filter (the walk without the test) ...

Every call is synchronous (it returns the dict of dicts), so the wall clock around it covers all device work.  kernel ms, pairs and rounds
come from the statistics block of the device search (isocon_nn_stats: kernel_ms, pairs_lanes, scan_launches, and the block test's
pairs_block_rejected, pairs_lanes_aligned, filter_kernel_ms); a build that answers such a call without the device search leaves them empty."""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Params(object):
    def __init__(self, depth):
        self.nr_cores = 1
        self.neighbor_search_depth = depth
        self.verbose = False
        self.develop_logfile = None


def main():
    args = sys.argv[1:]
    if args and args[0] == "--variant":
        os.environ["ISOCON_DEBUG_VARIANT"] = args[1]
        args = args[2:]
    which = args[0]
    depths = [int(x) for x in args[1:]] or [8]
    runs = int(os.environ.get("RUNS", "5"))
    spec = importlib.util.spec_from_file_location("make_golden_g19", os.path.join(ROOT, "tests", "golden", "make_golden_g19.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from isocon_amd import nearest_neighbor_graph as NNG
    X, C = mod.candidates(which)
    print("set %s: %d reads, %d candidates, variant %s" % (which, len(X), len(C), os.environ.get("ISOCON_DEBUG_VARIANT") or "-"), flush=True)
    for depth in depths:
        walls, kernels, filters, stats, edges = [], [], [], {}, 0
        for r in range(runs + 1):
            NNG.LAST_STATS.clear()
            t0 = time.perf_counter()
            g = NNG.compute_2set_nearest_neighbor_graph(X, C, Params(depth))
            dt = (time.perf_counter() - t0) * 1e3
            stats = dict(NNG.LAST_STATS)
            edges = sum(len(v) for v in g.values())
            if r:          # (the first call warms up: code objects, scratch pool)
                walls.append(dt)
                if "kernel_ms" in stats:
                    kernels.append(stats["kernel_ms"])
                    filters.append(stats.get("filter_kernel_ms", 0.0))
        line = "depth %d: wall median %.1f ms (min %.1f, max %.1f, %d runs), %d edges" % (depth, statistics.median(walls), min(walls), max(walls), runs, edges)
        if kernels:
            line += ", kernel median %.2f ms (min %.2f, max %.2f), %d pairs, %d rounds" % (statistics.median(kernels), min(kernels), max(kernels), stats.get("pairs_lanes", 0),
                                                                                             stats.get("scan_launches", 0))
            line += ", %d rejected by the block test, %d to the pair-per-lane launch, filter kernel median %.2f ms" % (
                stats.get("pairs_block_rejected", 0), stats.get("pairs_lanes_aligned", 0), statistics.median(filters))
        print(line, flush=True)


if __name__ == "__main__":
    main()
