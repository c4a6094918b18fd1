"""The designed inputs of tests/planted_cases.py are what they claim to be (CPU only: the oracle and the numpy restatements of the two
lower bounds): every planted pair is at exactly its distance, the bounds are tight where the cases say so, and every excursion pair's
optimal alignment is the one excursion, with the certificate on the side of its inequality that the case was built for."""
import re

import numpy as np

import planted_cases as PC
import qgram_ref as R
from oracle import oracle as O


def _distances(pairs):
    seqs, a, b = [], [], []
    for x, y in pairs:
        a.append(len(seqs)); b.append(len(seqs) + 1)
        seqs += [x, y]
    return O.ed_pairs(seqs, a, b, None).tolist()


def test_every_planted_pair_is_at_its_distance():
    cases = PC.planted_cases() + PC.full_pass_cases()
    assert _distances([(c.x, c.y) for c in cases]) == [c.d for c in cases]
    for c in cases:
        diff = len(c.y) - len(c.x)
        assert diff == {"del": -c.d, "ins": c.d, "sub": 0, "mix": c.d % 2}[c.kind], c.name
        if c.kind == "sub":          # a substituted base differs from the original: d mismatches, `spacing` apart
            at = np.flatnonzero(np.frombuffer(c.x.encode(), np.uint8) != np.frombuffer(c.y.encode(), np.uint8))
            assert len(at) == c.d and (np.diff(at) == c.spacing).all(), c.name
    # what the set is meant to hold
    small = PC.small_cases()
    assert {(c.d, c.kind, c.spacing) for c in small} == {(d, k, s) for d in (31, 32, 63, 64) for k in PC.KINDS for s in (8, 9, 16)}
    assert {c.d for c in cases} >= set(PC.EDGES + PC.TABLE_EDGES)
    assert {(c.d, c.kind) for c in PC.large_cases() if len(c.x) > c.d} == {(d, k) for d in PC.EDGES[2:] for k in PC.KINDS}
    assert {len(c.x) % 64 for c in small} == {63, 0, 1} and {len(c.x) % 64 for c in PC.large_cases() if len(c.x) > c.d} == {63, 0, 1}
    assert max(len(c.x) for c in PC.planted_cases()) <= 1601
    empty = [c for c in cases if c.y == ""]
    assert sorted(c.d for c in empty) == [32, 63, 64, 128, 512] and all(len(c.x) == c.d for c in empty)
    # the un-banded kernel's pattern is the SHORTER sequence: that one has the edge length, with every kind of partner
    full = PC.full_pass_cases()
    assert {(min(len(c.x), len(c.y)), c.kind) for c in full} == {(P, k) for P in (4095, 4096, 4097, 8193) for k in ("del", "ins", "sub")}
    assert len(full) == 12 and {c.d for c in full} == {512, 513} and all({c.d for c in full if c.kind == k} == {512, 513} for k in ("del", "ins", "sub"))


def test_every_group_partner_is_at_its_distance():
    groups = PC.group_cases()
    assert [len(p) for _, _, p in groups] == [1, 15, 16, 64, 65, 64]
    for name, x, partners in groups:
        assert _distances([(x, y) for y, _, _ in partners]) == [d for _, _, d in partners], name
        assert len({y for y, _, _ in partners}) == len(partners), name
    name, x, partners = groups[-1]
    diffs = [len(y) - len(x) for y, _, _ in partners]
    assert diffs == list(range(-63, 64, 2)) and [d for _, _, d in partners] == [abs(v) for v in diffs]
    # with k = d = |diff| a lane's path needs every diagonal between 0 and diff: together more than the 64 diagonals of one window
    assert max(diffs) - min(diffs) + 1 > 64


def test_nn_families_sit_on_their_edges():
    fams = PC.nn_families()
    assert [f.d for f in fams] == list(PC.TABLE_EDGES + PC.EDGES)
    signs = set()
    for f in fams:
        assert _distances([(f.base, s) for s, _ in f.members]) == [f.d] * 3, f.d
        assert _distances([(f.base, f.decoy)]) == [f.d + 1], f.d
        assert f.d <= min(len(s) for s, _ in f.members) and [k for _, k in f.members][1:] == ["sub", "mix"]
        signs.add(np.sign(len(f.members[0][0]) - len(f.base)))
    assert signs == {-1, 1}
    S, bases = PC.nn_set()
    assert len(S) == 5 * len(fams) < 100
    # the del / ins members at 63 and 64 and the decoys at 64 and 65 straddle the 63 bases of length difference the bound matrix covers
    by_d = {f.d: f for f in fams}
    assert abs(len(by_d[63].members[0][0]) - len(by_d[63].base)) == 63 and abs(len(by_d[64].members[0][0]) - len(by_d[64].base)) == 64
    assert abs(len(by_d[63].decoy) - len(by_d[63].base)) == 64
    # the block filter's comparison of count and threshold decides on a member whose count equals d (the threshold once another member
    # at d was found): at 31, 32 and 63 such a member exists -- in both directions and under both strides -- and at 31 and 32 the q-gram
    # bound of the substitution member equals d as well
    for d in (31, 32, 63):
        f = by_d[d]
        counts = [[R.block_count(*pair, s=s) for s in (4, 2) for pair in ((f.base, m), (m, f.base))] for m, _ in f.members]
        assert all(max(c) <= d for c in counts) and any(min(c) == d for c in counts), (d, counts)
        q = R.bound(R.profile(f.base), R.profile(f.members[1][0]))
        assert q <= d and (q == d or d == 63)


def test_both_lower_bounds_are_tight_on_spaced_edits():
    small = [c for c in PC.planted_cases() if c.d <= 64]
    prof = {c.name: (R.profile(c.x), R.profile(c.y)) for c in small}
    qb = {c.name: R.bound(*prof[c.name]) for c in small}
    blocks = {(c.name, s): (R.block_count(c.x, c.y, s=s), R.block_count(c.y, c.x, s=s)) for c in small for s in (4, 2)}
    for c in small:          # lower bounds, all of them
        assert qb[c.name] <= c.d and R.bound(*prof[c.name][::-1]) == qb[c.name], c.name
        assert all(max(blocks[c.name, s]) <= c.d for s in (4, 2)), c.name
    for d in (31, 32, 63):
        assert any(c.d == d and min(blocks[c.name, 4]) == d and min(blocks[c.name, 2]) == d for c in small), d          # both directions, both strides
    tight = [c.name for c in small if qb[c.name] == c.d]
    assert tight and any(n.startswith("sub_d32") for n in tight), tight


CIGAR = re.compile(r"(\d+)([=XID])")


def excursion_shape(cigar, g, trim):
    """True where the alignment is `a= gI b= gD c=` or its mirror, followed by the `trim` bases one sequence is longer at its end, with
    a + b + c all the other bases"""
    ops = [(int(n), c) for n, c in CIGAR.findall(cigar)]
    if trim:
        if len(ops) != 6 or ops[5][0] != trim or ops[5][1] not in "ID":
            return False
        ops = ops[:5]
    if len(ops) != 5 or [c for _, c in ops] not in (list("=I=D="), list("=D=I=")):
        return False
    return ops[1][0] == g and ops[3][0] == g and ops[0][0] + ops[2][0] + ops[4][0] == 2 * PC.FLANK + PC.MIDDLE - trim


def test_excursion_pairs_leave_the_diagonal_once_and_sit_on_the_certificate():
    cases = PC.excursion_cases()
    seen = set()
    for e in cases:
        h = e.hint
        m, n = len(e.s1), len(e.s2)
        assert m == 2 * PC.FLANK + PC.MIDDLE + e.g and n == m - h.trim
        assert PC.band_x(m, n, h.hint, h.mismatch, h.open, h.ext) == h.X and h.trim + 2 * h.X + 1 == e.target
        assert PC.band_x(n, m, h.hint, h.mismatch, h.open, h.ext) == h.X
        assert h.trim + 2 * h.X + 64 < n          # banded at all
        cost = PC.gap_cost(e.g, h.open, h.ext)
        for s1, s2 in ((e.s1, e.s2), (e.s2, e.s1)):
            for policy in (0, 21):
                r = O.sg_trace(s1, s2, PC.MATCH, h.mismatch, h.open, h.ext, policy)
                assert excursion_shape(r["cigar"], e.g, h.trim), (e.name, r["cigar"])
                assert r["score"] == PC.MATCH * (2 * PC.FLANK + PC.MIDDLE - h.trim) - 2 * cost, e.name
                # the certificate of csrc/sg_host.inc on that score: holds exactly when X >= g + the cost of one gap (open 2, ext 0: g + 2)
                certifies = r["score"] > PC.MATCH * (min(m, n) - h.X - 1)
                assert certifies == (h.X >= e.g + cost) == e.certifies, e.name
        assert h.X == e.g + cost - (0 if e.certifies else 1), e.name          # ... and sits next to the inequality, on either side
        seen.add((e.target, (h.open, h.ext), e.certifies))
    for target in PC.TARGET_DIAGS:
        assert (target, (2, 0), True) in seen and (target, (2, 0), False) in seen, target          # X == g + 2 and X == g + 1
        assert (target, (3, 0), True) in seen and (target, (3, 0), False) in seen, target
    assert tuple(e.name for e in cases if (e.hint.open, e.hint.ext) == (3, 1)) == PC.EXCURSIONS_3_1          # (all that exist under that model)
    # band_hint without a margin: some hint for every target, whatever g
    for target in PC.TARGET_DIAGS:
        h = PC.band_hint(target, 40)
        assert h is not None and h.trim + 2 * h.X + 1 == target
