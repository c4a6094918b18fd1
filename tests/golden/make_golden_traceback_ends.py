#!/usr/bin/env python3
"""Golden fixture tests/golden/g21_traceback_allow_ends.json: the reference's own
modules/end_invariant_functions.py::edlib_traceback_allow_ends (:191-223) on short pairs whose global alignment begins and / or ends
with an I or D run below, at and above the end threshold, for thresholds 0, 5 and 15.  edlib is the stand-in of tests/golden/shims
(the oracle's tie rule), which ignores k for task="path": every case carries a k at or above its distance, where edlib and the
stand-in agree.  Build container only."""
import contextlib
import io
import json
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def pairs():
    rng = random.Random(21)
    out = []
    for thr in (0, 5, 15):
        for lead, trail in [(0, 0), (thr, 0), (0, thr), (thr + 1, 0), (0, thr + 1), (max(thr - 1, 1), max(thr - 1, 1)), (thr, thr + 1), (thr + 1, thr),
                            (thr + 6, 0), (1, thr), (thr, thr), (0, 2 * thr + 3), (3, 0)]:
            # (the walk pushes a gap as far right as ties allow: a leading overhang stays ONE run only if none of its bases can be
            # matched further in -- the core begins with A / C only, the leading overhang is G / T only)
            core = "".join(rng.choice("AC") for _ in range(24)) + rnd(rng, rng.randint(30, 66))
            other = list(core)
            for _ in range(rng.choice([0, 1, 3])):          # internal differences, away from the ends
                p = rng.randrange(28, len(other) - 8)
                r = rng.random()
                if r < 0.4:
                    other[p] = rng.choice("ACGT")
                elif r < 0.7:
                    del other[p]
                else:
                    other.insert(p, rng.choice("ACGT"))
            x, y = core, "".join(other)
            if rng.random() < 0.5:          # the overhang on the query (I) or on the target (D)
                x = "".join(rng.choice("GT") for _ in range(lead)) + x
            else:
                y = "".join(rng.choice("GT") for _ in range(lead)) + y
            if rng.random() < 0.5:
                x = x + rnd(rng, trail)
            else:
                y = y + rnd(rng, trail)
            out.append((x, y, thr))
    out += [("ACGT", "ACGT", 5), ("ACG", "", 5), ("", "ACGTACG", 5), ("ACGTACGTAC", "TTTTTTTTTT", 15)]
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(HERE, "shims"))
    sys.path.insert(0, REF)
    import networkx
    if not hasattr(networkx.Graph, "node"):
        networkx.Graph.node = property(lambda g: g.nodes)
    with contextlib.redirect_stdout(io.StringIO()):
        from modules import end_invariant_functions as R_END
    import edlib
    rng = random.Random(3)
    cases, seen = [], set()
    for x, y, thr in pairs():
        full = edlib.align(x, y, mode="NW", task="path")
        k = full["editDistance"] + rng.choice([0, 0, 1, 7])
        ed, locations, cigar = R_END.edlib_traceback_allow_ends(x, y, mode="NW", task="path", k=k, end_threshold=thr)
        cases.append({"x": x, "y": y, "k": k, "end_threshold": thr, "ed": ed, "locations": [list(l) for l in locations], "cigar": cigar})
        runs = re.findall(r"(\d+)([=XID])", cigar or "")
        for where, (n, op) in (("lead", runs[0]), ("trail", runs[-1])) if runs else ():
            if op in "ID":
                seen.add((thr, where, "below" if int(n) < thr else "at" if int(n) == thr else "above"))
    for thr in (5, 15):
        for where in ("lead", "trail"):
            assert {(thr, where, c) for c in ("below", "at", "above")} <= seen, (thr, where, sorted(seen))
    assert {(0, "lead", "above"), (0, "trail", "above")} <= seen
    json.dump({"generator": "tests/golden/make_golden_traceback_ends.py", "cases": cases}, open(os.path.join(HERE, "g21_traceback_allow_ends.json"), "w"), indent=0)
    print(len(cases), "cases", sum(c["ed"] != edlib.align(c["x"], c["y"], mode="NW", task="path")["editDistance"] for c in cases), "with a forgiven end run")


if __name__ == "__main__":
    main()
