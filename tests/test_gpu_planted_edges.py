"""The distance, bound, nearest-neighbour and alignment kernels on the designed inputs of tests/planted_cases.py: pairs whose distance is
the last value a rung of the band ladder holds or the first it does not (31 / 32, 63 / 64, 127 / 128, 255 / 256, 511 / 512), groups at
the 16-pair and 64-lane switches of isocon_ed_pairs, the un-banded kernel around its 4096-row pass, lower bounds that equal the
distance, neighbours that tie on an edge with a decoy one edit behind, and alignments whose band is 127 .. 129 and 255 .. 257 diagonals
wide with the optimal path next to its edge and the certificate on either side of its inequality.  Everything is compared with the
oracle (tests/test_planted_cases.py shows on the CPU that the inputs sit where they claim to); all comparisons are exact."""
import re

import numpy as np
import pytest

import planted_cases as PC
import qgram_ref as R
from conftest import Params, ordered
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CIGAR = re.compile(r"(\d+)([=XID])")
ROUTINGS = (None, "ed_lanes=1", "ed_lanes=0")          # default (fewer than 16 pairs per shared sequence: one pair per lane), all / none per lane


def _variant(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    else:
        monkeypatch.setenv("ISOCON_DEBUG_VARIANT", value)


def _expected(d, k):
    return d if k < 0 or k >= d else -1


# ---- a. isocon_ed_pairs at every rung -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """the planted pairs in one store with the oracle's answers to k = d - 1, d, d + 1 and unbounded in both argument orders, computed once"""
    from isocon_amd.store import SeqStore
    cases = PC.planted_cases()
    seqs, a, b, k, want = [], [], [], [], []
    for c in cases:
        i = len(seqs)
        seqs += [c.x, c.y]
        for kk in (c.d - 1, c.d, c.d + 1, -1):
            for u, v in ((i, i + 1), (i + 1, i)):
                a.append(u); b.append(v); k.append(kk); want.append(_expected(c.d, kk))
    exp = O.ed_pairs(seqs, a, b, k)
    assert exp.tolist() == want          # -1 at d - 1, d at d, d + 1 and unbounded
    st = SeqStore(seqs)
    yield cases, seqs, np.asarray(a), np.asarray(b), np.asarray(k), exp, st
    st.close()


@pytest.mark.parametrize("routing", ROUTINGS)
def test_ed_pairs_planted_distances_at_every_rung(planted, routing, monkeypatch):
    cases, seqs, a, b, k, exp, st = planted
    _variant(monkeypatch, routing)
    got = st.ed_pairs(a, b, k)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, [(cases[i // 8].name, int(k[i]), int(exp[i]), int(got[i])) for i in bad[:10]]
    # one threshold per call: every shared sequence has one pair (the default routing takes the other branch than above where a call mixes them)
    for slot in range(4):
        sel = np.flatnonzero(np.arange(len(k)) % 8 // 2 == slot)
        got = st.ed_pairs(a[sel], b[sel], k[sel])
        assert (got == exp[sel]).all(), slot
    assert (st.ed_pairs(a, b, None) == np.repeat([c.d for c in cases], 8)).all()


@pytest.fixture(scope="module")
def groups():
    from isocon_amd.store import SeqStore
    gs = PC.group_cases()
    seqs, shared, partner, d = [], [], [], []
    for name, x, partners in gs:
        i = len(seqs)
        seqs.append(x)
        for y, kind, dd in partners:
            shared.append(i); partner.append(len(seqs)); d.append(dd)
            seqs.append(y)
    d = np.asarray(d)
    assert O.ed_pairs(seqs, shared, partner, None).tolist() == d.tolist()
    st = SeqStore(seqs)
    yield seqs, np.asarray(shared), np.asarray(partner), d, st
    st.close()


@pytest.mark.parametrize("routing", ROUTINGS)
def test_ed_pairs_group_sizes_and_spread_length_differences(groups, routing, monkeypatch):
    """one shared sequence with 1, 15, 16, 64 and 65 partners (one pair per lane below 16; one tile of 64 lanes, then a second), and 64 partners
    whose length differences run from -63 to +63: with k = d their bands together span 127 diagonals, which no window of 64 holds.
    One threshold per call, so that a shared sequence has exactly as many pairs as partners; both argument orders (the shared side is
    found by counting)."""
    seqs, shared, partner, d, st = groups
    _variant(monkeypatch, routing)
    for dk in (-1, 0, 1, None):
        k = np.full(len(d), -1) if dk is None else d + dk
        want = np.where((k < 0) | (k >= d), d, -1)
        exp = O.ed_pairs(seqs, shared, partner, k)
        assert exp.tolist() == want.tolist()
        assert st.ed_pairs(shared, partner, k).tolist() == exp.tolist(), dk
        assert st.ed_pairs(partner, shared, k).tolist() == exp.tolist(), dk


# ---- b. the un-banded kernel around its 4096-row pass -----------------------------------------------------------------------------------------

def test_ed_full_at_the_pass_edge():
    """pattern (the shorter sequence) of 4095, 4096, 4097 (one pass, its last row, the first row of a second pass) and 8193 bases (the first
    row of a third), each with a deletion, an insertion and a substitution partner at distance 512 or 513, which no band holds:
    k = d - 1, d and unbounded, both argument orders"""
    from isocon_amd.store import SeqStore
    cases = PC.full_pass_cases()
    seqs, a, b, k, want = [], [], [], [], []
    for c in cases:
        i = len(seqs)
        seqs += [c.x, c.y]
        for kk in (c.d - 1, c.d, -1):
            for u, v in ((i, i + 1), (i + 1, i)):
                a.append(u); b.append(v); k.append(kk); want.append(_expected(c.d, kk))
    exp = O.ed_pairs(seqs, a, b, k)
    assert exp.tolist() == want
    st = SeqStore(seqs)
    try:
        got = st.ed_pairs(a, b, k)
        assert got.tolist() == exp.tolist(), [(cases[i // 6].name, k[i], int(exp[i]), int(got[i])) for i in np.flatnonzero(got != exp)[:10]]
    finally:
        st.close()


# ---- c. the two lower bounds through the ABI ----------------------------------------------------------------------------------------------------

def test_bounds_equal_the_restatement_and_are_tight_where_it_is(planted):
    cases, seqs, a, b, k, exp, st = planted
    small = [(i, c) for i, c in enumerate(cases) if c.d <= 64]
    x = np.asarray([2 * i for i, _ in small], dtype=np.uint32)
    y = x + 1
    d = np.asarray([c.d for _, c in small])
    prof = [(R.profile(c.x), R.profile(c.y)) for _, c in small]
    want_q = np.asarray([R.bound(p, q) for p, q in prof])
    for u, v in ((x, y), (y, x)):
        got = st.qgram_bound_pairs(u, v)
        assert (got == want_q).all() and (got <= d).all()
    tight_q = [c.name for (_, c), q in zip(small, want_q) if q == c.d]
    assert any(n.startswith("sub_d32") for n in tight_q) and any(n.startswith("sub_d31") for n in tight_q), tight_q
    tight = {s: np.ones(len(small), dtype=bool) for s in (4, 2)}
    for stride in (4, 2):
        for owner, partner, swap in ((x, y, False), (y, x, True)):
            got = st.block_bound_pairs(owner, partner, probe_stride=stride)
            want = np.asarray([R.block_count(*((c.y, c.x) if swap else (c.x, c.y)), s=stride) for _, c in small])
            assert (got == want).all(), (stride, swap, np.flatnonzero(got != want)[:10])
            assert (got <= d).all()
            tight[stride] &= got == d
    for dd in (31, 32, 63):          # a bound that equals the distance in both directions under both strides: `>` against `>=` decides there
        assert ((d == dd) & tight[4] & tight[2]).any(), dd


# ---- d. - f. neighbours on the edge -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nn_world():
    """the families with the oracle's graphs, computed once"""
    S, bases = PC.nn_set()
    conv = set(S[acc] for acc in bases)
    g_cpu, iso_cpu = O.compute_nearest_neighbor_graph(S, set(), Params(1))
    g_conv, iso_conv = O.compute_nearest_neighbor_graph(S, conv, Params(1))
    # the cases sit where they are meant to: every base's neighbours are its three members, tied at d; the decoy at d + 1 is not among them
    for acc, d in bases.items():
        assert g_cpu[acc] == {"%s%d" % (kind, d): d for _, kind in [f for f in PC.nn_families() if f.d == d][0].members}, acc
        assert g_conv[acc] == {}
    return S, bases, conv, (g_cpu, iso_cpu), (g_conv, iso_conv)


# (the del / ins members at d = 63 and 64 and their decoys at 64 and 65 straddle the +-63 bases of length difference that the bound matrix
# and the 64-row main pass cover: 63 is the last neighbour the main pass may resolve, 64 the first that belongs to the wide phase)
@pytest.mark.parametrize("variant", [None, "nn_no_qgram=1", "nn_no_block_filter", "nn_narrow=1"])
def test_nn_graph_with_neighbours_on_every_edge(nn_world, variant, monkeypatch):
    from isocon_amd import nearest_neighbor_graph as NNG
    S, bases, conv, (g_cpu, iso_cpu), (g_conv, iso_conv) = nn_world
    _variant(monkeypatch, variant)
    g_gpu, iso_gpu = NNG.compute_nearest_neighbor_graph(S, set(), Params(1))
    stats = dict(NNG.LAST_STATS)
    assert ordered(g_gpu) == ordered(g_cpu) and iso_gpu == iso_cpu
    if variant == "nn_no_qgram=1":
        assert stats["pairs_prefiltered"] == 0
    if variant == "nn_no_block_filter":
        assert stats["pairs_block_rejected"] == 0
    g_gpu, iso_gpu = NNG.compute_nearest_neighbor_graph(S, conv, Params(1))          # the bases converged: no rows of their own, still neighbours
    assert ordered(g_gpu) == ordered(g_conv) and iso_gpu == iso_conv


def test_nn_sharded_phases_equal_the_single_call_and_the_oracle(nn_world):
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore, nn_finalize
    S = nn_world[0]
    seqs = sorted(S.values(), key=len)
    n = len(seqs)
    packed = O.pack(seqs)
    row_ptr, cols, eds, _ = O.nn_1set(seqs, np.zeros(n, np.uint8), 0, n, packed=packed)
    st = SeqStore(seqs)
    try:
        best1, rp1, cols1, _ = st.nn_graph()
        assert rp1.tolist() == row_ptr.tolist() and cols1.tolist() == cols.tolist()
        assert np.repeat(best1, np.diff(rp1)).tolist() == eds.tolist()
        shards = [(8 * r, n, 24, 8) for r in range(3)]          # block-cyclic: blocks of 8 entries dealt to three ranks
        for phases in ((0, 1, 2), (3, 2)):
            hits = []
            red = np.full(n, _lib.NN_INF, dtype=np.int32)
            for phase in phases:
                bests = []
                for (b, e, stride, block) in shards:
                    best = red.copy()
                    h, _ = st.nn_partial(b, e, phase, best, q_stride=stride, q_block=block)
                    bests.append(best); hits.append(h)
                red = np.minimum.reduce(bests)
            best2, rp2, cols2 = nn_finalize(n, red, np.concatenate(hits))
            assert best2.tolist() == best1.tolist() and rp2.tolist() == rp1.tolist() and cols2.tolist() == cols1.tolist(), phases
    finally:
        st.close()


def test_nn_2set_with_candidates_on_every_edge(nn_world):
    """the members and decoys as reads, the bases as candidates, and a read that IS a candidate (distance 0 is admitted)"""
    from isocon_amd import nearest_neighbor_graph as NNG
    S, bases = nn_world[:2]
    X = {acc: s for acc, s in S.items() if acc not in bases}
    C = {acc: S[acc] for acc in bases}
    X["same_as_base63"] = S["base63"]
    for depth in (2 ** 32, 1):
        g_cpu = O.compute_2set_nearest_neighbor_graph(X, C, Params(1, depth))
        if depth > 1:
            assert g_cpu["same_as_base63"] == {"base63": 0}
            for acc, d in bases.items():
                assert g_cpu["sub%d" % d] == {acc: d} and g_cpu["mix%d" % d] == {acc: d} and g_cpu["decoy%d" % d] == {acc: d + 1}
        g_gpu = NNG.compute_2set_nearest_neighbor_graph(X, C, Params(1, depth))
        assert ordered(g_gpu) == ordered(g_cpu), depth


# ---- g. alignment band classes ------------------------------------------------------------------------------------------------------------------------

def restated_band(m, n, hint, mismatch, open_, ext, match):
    """csrc/sg_host.inc: the half-width X from an edit-distance hint and the band's diagonals |D| + 2 X + 1 (None: not banded)"""
    aD = abs(n - m)
    Q = max(-mismatch, open_ + ext)
    X = ((match + Q) * hint + match - 1) // match - aD + 1
    if X < 1:
        X = 1
    if not aD + 2 * X + 64 < min(m, n):
        return None
    return X, aD + 2 * X + 1


def _gapped(s1, s2, cigar):
    a1, a2, i, j = [], [], 0, 0
    for n, c in CIGAR.findall(cigar):
        n = int(n)
        if c in "=X":
            a1.append(s1[i:i + n]); a2.append(s2[j:j + n]); i += n; j += n
        elif c == "I":
            a1.append(s1[i:i + n]); a2.append("-" * n); i += n
        else:
            a1.append("-" * n); a2.append(s2[j:j + n]); j += n
    assert i == len(s1) and j == len(s2)
    return "".join(a1), "".join(a2)


class Excursions(object):
    """the excursion pairs in one store; the oracle's alignments (no hints) per (case, argument order, tie policy), computed on first use"""

    def __init__(self):
        from isocon_amd.store import SeqStore
        self.cases = PC.excursion_cases()
        self.seqs = [s for e in self.cases for s in (e.s1, e.s2)]
        self.st = SeqStore(self.seqs)
        self._want = {}
        for e in self.cases:          # the restated formula puts every pair on its target: a change of the library's formula moves the classes below
            h = e.hint
            assert restated_band(len(e.s1), len(e.s2), h.hint, h.mismatch, h.open, h.ext, PC.MATCH) == (h.X, e.target), e.name
            assert restated_band(len(e.s2), len(e.s1), h.hint, h.mismatch, h.open, h.ext, PC.MATCH) == (h.X, e.target), e.name

    def want(self, i, swap, policy):
        key = (i, swap, policy)
        if key not in self._want:
            e = self.cases[i]
            s1, s2 = (e.s2, e.s1) if swap else (e.s1, e.s2)
            self._want[key] = O.sg_trace(s1, s2, PC.MATCH, e.hint.mismatch, e.hint.open, e.hint.ext, policy)
        return self._want[key]

    def run(self, sel, policy, strings=False):
        """the cases `sel` in both argument orders with their hints, one call per gap model: every result against the oracle; the counters
        of the calls, summed"""
        from isocon_amd import SW_alignment_module as SWM
        from isocon_amd.store import sg_last_stats
        total = {}
        for model in PC.GAP_MODELS:
            idx = [i for i in sel if (self.cases[i].hint.open, self.cases[i].hint.ext) == model]
            if not idx:
                continue
            a = [2 * i + sw for i in idx for sw in (0, 1)]
            b = [2 * i + 1 - sw for i in idx for sw in (0, 1)]
            mm = np.asarray([self.cases[i].hint.mismatch for i in idx for sw in (0, 1)], dtype=np.int8)
            hints = np.asarray([self.cases[i].hint.hint for i in idx for sw in (0, 1)], dtype=np.int32)
            if strings:
                sa, sb, sp, res, ops, ptr = self.st.sg_strings(a, b, mm, match=PC.MATCH, open_=model[0], ext=model[1], tie_policy=policy, return_ops=True, ed_upper=hints)
                sa, sb = bytes(sa).decode(), bytes(sb).decode()
            else:
                ops, ptr, res = self.st.sg_trace(a, b, mm, match=PC.MATCH, open_=model[0], ext=model[1], tie_policy=policy, ed_upper=hints)
            for key, v in sg_last_stats().items():
                total[key] = total.get(key, 0) + v
            for p in range(len(a)):
                i, swap = idx[p // 2], p % 2
                exp = self.want(i, swap, policy)
                got = dict(cigar=SWM.ops_to_cigar(ops[ptr[p]:ptr[p + 1]].tolist()), score=int(res[p, 0]), end_query=int(res[p, 1]), end_ref=int(res[p, 2]),
                           matches=int(res[p, 3]), mismatches=int(res[p, 4]), indels=int(res[p, 5]))
                assert got == exp, (self.cases[i].name, swap, policy, got, exp)
                if strings:
                    assert (sa[sp[p]:sp[p + 1]], sb[sp[p]:sp[p + 1]]) == _gapped(self.seqs[a[p]], self.seqs[b[p]], exp["cigar"]), (self.cases[i].name, swap, policy)
        return total


@pytest.fixture(scope="module")
def excursions():
    w = Excursions()
    yield w
    w.st.close()


@pytest.mark.parametrize("policy", [0, 21])
def test_alignment_band_classes_with_the_path_next_to_the_edge(excursions, policy, monkeypatch):
    """Every excursion pair equals the oracle's hint-free alignment, and the counters show the class its band belongs to: 127 and 128
    diagonals two per lane, 129, 255 and 256 four per lane, 257 in strips; a pair one diagonal short of its certificate is aligned again
    in full, a pair that just has it is not."""
    w = excursions
    certified = lambda targets: [i for i, e in enumerate(w.cases) if e.target in targets and e.certifies]
    _variant(monkeypatch, None)
    sel = certified((127, 128))
    stats = w.run(sel, policy)
    assert stats["pairs_band_narrow"] == stats["pairs_band"] == 2 * len(sel) > 0 and stats["pairs_strips"] == 0 and stats["pairs_redone"] == 0, stats
    sel = certified((129, 255, 256))
    stats = w.run(sel, policy)          # with the narrow try: 129 diagonals are tried on 128 and run again wider (the try misses the certificate by one)
    assert stats["pairs_redone"] == 0 and stats["pairs_strips"] == 0 and stats["pairs_retried_wider"] > 0, stats
    _variant(monkeypatch, "sw_no_narrow_try")
    stats = w.run(sel, policy)
    assert stats["pairs_band"] == 2 * len(sel) > 0 and stats["pairs_band_narrow"] == 0 and stats["pairs_strips"] == 0 and stats["pairs_redone"] == 0, stats
    assert stats["pairs_tried_narrow"] == 0
    _variant(monkeypatch, None)
    sel = certified((257,))
    stats = w.run(sel, policy)
    assert stats["pairs_strips"] == 2 * len(sel) > 0 and stats["pairs_band"] == 0 and stats["pairs_redone"] == 0, stats
    # one diagonal short: the banded result is not certified and the pair is aligned again in full (which the strips count too)
    for targets in ((127, 128), (129, 255, 256), (257,)):
        sel = [i for i, e in enumerate(w.cases) if e.target in targets and not e.certifies]
        for variant in (None, "sw_no_narrow_try"):
            _variant(monkeypatch, variant)
            stats = w.run(sel, policy)
            assert stats["pairs_redone"] == 2 * len(sel) > 0, (targets, variant, stats)
    _variant(monkeypatch, None)
    everything = list(range(len(w.cases)))
    stats = w.run(everything, policy)
    assert stats["pairs_redone"] == 2 * sum(not e.certifies for e in w.cases), stats


@pytest.mark.parametrize("policy", [0, 21])
def test_gapped_strings_of_the_excursion_pairs(excursions, policy, monkeypatch):
    w = excursions
    _variant(monkeypatch, None)
    stats = w.run([i for i, e in enumerate(w.cases) if e.certifies], policy, strings=True)          # one batch, nothing to redo: expanded in place
    assert stats["pairs_redone"] == 0
    stats = w.run(list(range(len(w.cases))), policy, strings=True)                                  # with pairs that are aligned again
    assert stats["pairs_redone"] == 2 * sum(not e.certifies for e in w.cases)
