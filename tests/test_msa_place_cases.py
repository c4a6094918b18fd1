"""CPU: the partitions of tests/msa_place_cases.py still have the properties tests/test_gpu_msa_place.py relies on."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msa_place_cases as PC  # noqa: E402


def test_the_cases_hold_what_they_were_built_for():
    P, plan = PC.build_partitions()
    steps = set()
    for t, rep, q, step in P["outcomes"].outcome_pairs:          # each of the four steps of the rule, by the anchor, with rep the slot's representative
        assert PC.anchor(rep, q)[1] == step and min(x for x in (rep, q) if len(x) == len(rep)) == rep
        steps.add(step)
    assert steps == {PC.SUBSTRING, PC.THREADED, PC.OFFSET, PC.LEFT}
    longest = P["lengths"].host()[1]
    assert sorted(int(x) for x in longest[longest > 1]) == [2, 3, 5, 32, 33, 62, 63, 64, 70] and longest[0] == 2 and longest[300] == 5
    for t in np.flatnonzero(longest > 1):
        lens = [len(s) for _, tt, s in P["lengths"].insertions() if tt == t]
        assert 1 in lens and int(longest[t]) in lens          # m = 1 and m = longest in one slot
    tails = [s for r, t, s in P["behind_base_32"].insertions() if t == 30 and r <= 4]
    assert len({s[:32] for s in tails}) == 1 and len(set(tails)) == 4 and {len(s) for s in tails} == {42} and tails[0] != min(tails)
    assert P["behind_base_32"].host()[1][30] == 42 and P["behind_base_32"].host()[1][80] == 62
    ins = P["many_rows"].insertions()
    assert sum(1 for _, t, s in ins if t == 40 and s == "ACCA") > 64 and len({s for _, t, s in ins if t == 60}) > 64
    a, b = P["twin_a"], P["twin_b"]
    assert a.host()[1][33] == b.host()[1][33] == 6 and min(s for _, t, s in a.insertions() if len(s) == 6) != min(s for _, t, s in b.insertions() if len(s) == 6)
    assert (P["no_wide_slot"].host()[1] <= 1).all()
    ops = P["many_ops"].ops[0]
    wide_at = [k for k, o in enumerate(ops) if int(o) & 15 == 3 and int(o) >> 4 > 1]
    assert len(ops) > 64 and min(wide_at) < 64 <= max(wide_at)
    assert all(p.n_rows <= 70 and len(p.centre) <= 1100 for p in P.values())
    assert sorted(P) == sorted(PC.ORDER) and set(plan) == set(P)
