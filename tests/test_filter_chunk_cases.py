"""CPU: the designed chunks of tests/filter_chunk_cases.py sit where they claim -- from the restatement alone, no library -- and a
restatement that is wrong in one place gives another answer on at least one of them (which stands in for a kernel that is wrong there:
tests/test_gpu_filter_chunks.py compares the device with the restatement on the same chunks)."""
import operator
import os
import re
from collections import Counter

import numpy as np
import pytest

from tests import filter_chunk_cases as F
from tests import qgram_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(call, second):
    """(owner, partner, word, k, count4, count2, chunk result) of every pair of a call"""
    exp = F.expected(call.name, second)
    for (owner, narrow, words), res in zip(call.chunks, exp["per_chunk"]):
        for w in words:
            w = int(w)
            y = w & F.INDEX_MASK
            yield owner, y, w, F.pair_threshold(w, call.thr, owner, call.kcap), F.count(call.seqs[owner], call.seqs[y], 4), F.count(call.seqs[owner], call.seqs[y], 2), res


def test_restated_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "isocon_amd", "csrc", "nn_filter.hpp")).read() + open(os.path.join(ROOT, "isocon_amd", "csrc", "nn_list.hpp")).read()

    def const(name):
        m = re.search(r"\b%s = ([0-9 *+]+);" % name, text) or re.search(r"#define ISOCON_%s ([0-9]+)" % name, text)
        return eval(m.group(1))
    assert const("NNF_GRID") == F.NNF_GRID and const("NNF_GRID2") == F.NNF_GRID2 and const("NNF_PASS2_MIN") == F.PASS2_MIN
    assert const("NN_LIST_MIN") == F.LIST_MIN and const("NN_LIST_CHUNK") + 63 == F.CHUNK_MAX and const("NNF_BATCH") == F.PIECE


def test_every_call_is_well_formed():
    total = 0
    for call in F.cases().values():
        n = len(call.seqs)
        assert len(call.thr) == n and call.thr.min() >= 0 and call.thr.max() <= 64 and max(map(len, call.seqs)) <= 600
        pairs = [(o, int(w) & F.INDEX_MASK) for o, _, words in call.chunks for w in words]
        assert len(set(pairs)) == len(pairs), call.name          # results compare as sets
        assert all(0 <= o < n and 1 <= len(words) <= F.CHUNK_MAX and narrow in (0, 1) for o, narrow, words in call.chunks)
        assert all(p < n for _, p in pairs)
        owners_of = {}
        for o, p in pairs:
            owners_of.setdefault(p, set()).add(o)
        if call.name != "early_exit" and not call.name.startswith("edge_k/"):
            assert max(map(len, owners_of.values())) >= 2, call.name          # the same partner under two owners
        total += len(pairs)
    # (most of them in the queue case -- more tasks than 4 NNF_GRID2, of at least 16 pairs each -- whose texts are short: the restatement stays at seconds)
    assert total < 200000


def test_routing_reaches_every_branch_on_both_sides():
    call = F.cases()["routing"]
    lm = call.list_min
    for second, routes in ((1, ("table", "second", "flat")), (0, ("table", "flat"))):
        exp = F.expected("routing", second)
        seen = Counter((narrow, r.route) for (_, narrow, _), r in zip(call.chunks, exp["per_chunk"]))
        assert all(seen[narrow, route] >= 3 for narrow in (0, 1) for route in routes), seen
        assert not second or not [k for k in seen if k[1] not in routes]
    exp = F.expected("routing", 1)
    for narrow in (0, 1):
        shapes = {(len(words), r.np) for (_, nr, words), r in zip(call.chunks, exp["per_chunk"]) if nr == narrow}
        nps = {np_ for _, np_ in shapes}
        assert {lm - 1, lm, 15, 16, 64, 65, 129, 0} <= nps, nps
        assert {-1, 0, 1} <= {2 * np_ - cnt for cnt, np_ in shapes if np_ >= lm}
    # the survivors of the first pass are what the case planned (the partners' counts are 2 on both grids)
    planned = [kept for _ in range(4) for _, kept in F.ROUTING_SHAPES]
    assert [r.np for r in exp["per_chunk"]] == planned


def test_edge_k_sits_on_both_sides_of_every_threshold():
    at_k, above_k = Counter(), Counter()              # (stride, count): pairs at count == k, at count == k + 1
    sources = Counter()
    only_second = finer_smaller = no_bits = 0
    for name in ("edge_k/partner", "edge_k/owner", "edge_k/kcap"):
        call = F.cases()[name]
        for o, y, w, k, c4, c2, res in _pairs(call, 1):
            ko, ky = int(call.thr[o]), int(call.thr[y])
            both = (w & F.OWNER_BIT) and (w & F.PARTNER_BIT)
            src = ("kcap" if k == call.kcap and min(ko if w & F.OWNER_BIT else 99, ky if w & F.PARTNER_BIT else 99) > call.kcap else
                   "both, owner larger" if both and ko > ky else "both, partner larger" if both and ky > ko else
                   "owner" if w & F.OWNER_BIT and not both else "partner" if w & F.PARTNER_BIT and not both else "other")
            if k == -1:
                no_bits += c4 == 0
                continue
            if c4 in (k, k + 1):
                (at_k if c4 == k else above_k)[4, c4] += 1
                sources[src, c4 == k] += 1
            if res.route == "second" and c4 <= k:
                if c2 in (k, k + 1):
                    (at_k if c2 == k else above_k)[2, c2] += 1
                only_second += c2 > k
                finer_smaller += c2 < c4
    for s in (4, 2):
        assert sum(v for (st, _), v in at_k.items() if st == s) >= 20 and sum(v for (st, _), v in above_k.items() if st == s) >= 20
        for c in (0, 1, 31, 32, 63):
            assert at_k[s, c] >= 1, (s, c, sorted(at_k))              # kept at k = c ...
            assert c == 0 or above_k[s, c] >= 1, (s, c, sorted(above_k))          # ... rejected at k = c - 1
    assert no_bits >= 1              # count 0 and still rejected: a word with neither bit
    assert only_second >= 50 and finer_smaller >= 1, (only_second, finer_smaller)
    for src in ("owner", "partner", "both, owner larger", "both, partner larger", "kcap"):
        assert sources[src, True] >= 1 and sources[src, False] >= 1, (src, sources)


def test_lengths_cover_the_dword_and_piece_steps():
    call = F.cases()["lengths"]
    partner_lengths = {len(call.seqs[int(w) & F.INDEX_MASK]) for _, _, words in call.chunks for w in words}
    assert set(F.LENGTHS + F.LENGTHS_2) <= partner_lengths
    for s in (4, 2):          # the listed lengths lie on both sides of a step of the dword count and of a piece
        nd = {F.dwords(L, s) for L in F.LENGTHS + F.LENGTHS_2}
        assert {0, 1, 2, 15, 16, 17, 18, 31, 32} <= nd, (s, sorted(nd))
        assert {F.pieces(L, s) for L in F.LENGTHS} == {0, 1, 2}
    owners = [call.seqs[o] for o, _, _ in call.chunks]
    assert set(range(0, 9)) <= set(map(len, owners)) and "A" * 300 in owners and any(len(x) == 300 and x != "A" * 300 for x in owners)
    assert any(x in (call.seqs[int(w) & F.INDEX_MASK] for w in words) for x, (_, _, words) in zip(owners, call.chunks))          # an exact copy of a partner
    for _, _, words in call.chunks:
        waves = [[len(call.seqs[int(w) & F.INDEX_MASK]) for w in words[i:i + 64]] for i in range(0, len(words), 64)]
        # the first wave: one lane's text is a whole piece longer than every other lane's, on both grids
        for s in (4, 2):
            p = sorted(F.pieces(L, s) for L in waves[0])
            assert len(p) == 64 and p[-1] == 2 and p[-2] <= 1
        assert all(len({F.dwords(L, 4) for L in wv}) > 4 for wv in waves[1:])          # the others mix
    # the decisions are not one-sided, and the second pass sees these lengths too
    exp = F.expected("lengths", 1)
    assert exp["f_tasks"] > 0 and 0.2 < exp["f_rejected"] / sum(len(w) for _, _, w in call.chunks) < 0.8


def test_early_exit_waves():
    call = F.cases()["early_exit"]
    exp = F.expected("early_exit", 1)
    (o, _, w_first), (_, _, w_g0), (_, _, w_g1) = call.chunks
    x = call.seqs[o]

    def lanes(words, s):
        """per lane: (k, count in the first piece, whole count)"""
        return [(F.pair_threshold(int(w), call.thr, o, call.kcap), F.first_piece_count(x, call.seqs[int(w) & F.INDEX_MASK], s), F.count(x, call.seqs[int(w) & F.INDEX_MASK], s))
                for w in words]
    w0, w1, w2 = (lanes(w_first[i:i + 64], 4) for i in (0, 64, 128))
    assert all(first > k for k, first, _ in w0)                                    # every lane rejected in the first piece: the loop may stop there
    for wave, kept in ((w1, False), (w2, True)):
        late = [(k, first, whole) for k, first, whole in wave if first <= k]
        assert len(late) == 1 and late[0][1] == 0 and late[0][2] == 1 and (late[0][2] <= late[0][0]) == kept          # one lane decided by its last dword
    assert exp["per_chunk"][0].np == 1
    # the second pass: every lane passed the first; 63 are rejected in the first piece of the 2-base grid, one is decided at the end of its text
    for words, res, kept in ((w_g0, exp["per_chunk"][1], False), (w_g1, exp["per_chunk"][2], True)):
        assert res.route == "second" and res.np == 64 and int(res.final.sum()) == int(kept)
        late = [(k, first, whole) for k, first, whole in lanes(words, 2) if first <= k]
        assert len(late) == 1 and late[0][1] == 0 and late[0][2] == 2 and (late[0][2] <= late[0][0]) == kept


def test_sizes_and_queue():
    for name, lm in (("sizes/list_min_256", 256), ("sizes/list_min_32", 32)):
        call = F.cases()[name]
        assert tuple(len(w) for _, _, w in call.chunks) == F.SIZES and call.list_min == lm and F.SIZES[-1] == F.CHUNK_MAX
        assert len({r.route for r in F.expected(name, 1)["per_chunk"]}) == 3
    call = F.cases()["queue"]
    exp = F.expected("queue", 1)
    assert len(call.chunks) > F.NNF_GRID and exp["f_tasks"] > 4 * F.NNF_GRID2
    assert sum(32 <= len(w) <= 40 for _, _, w in call.chunks) >= 2200
    assert exp["f_rejected"] > 10000 and exp["f_rejected2"] > 1000 and exp["n_small"] > 50000
    # consecutive chunks: owners without a common gram
    grams = lambda s: {s[i:i + 8] for i in range(len(s) - 7)}
    assert all(not grams(call.seqs[call.chunks[c][0]]) & grams(call.seqs[call.chunks[c + 1][0]]) for c in range(0, 200))


def test_the_count_is_a_lower_bound_of_the_distance():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    checked = 0
    for name in ("lengths", "edge_k/partner", "early_exit", "sizes/list_min_32", "queue"):
        call = F.cases()[name]
        pairs = [(o, int(w) & F.INDEX_MASK) for o, _, words in call.chunks for w in words]
        for i in rng.choice(len(pairs), 120, replace=False):
            a, b = call.seqs[pairs[i][0]], call.seqs[pairs[i][1]]
            d = O.ed_bounded(a, b) if a and b else max(len(a), len(b))
            assert F.count(a, b, 4) <= d and F.count(a, b, 2) <= d, (name, pairs[i])
            checked += 1
    assert checked == 600


# ---- one wrong piece at a time ---------------------------------------------------------------------------------------------------------

def _count_variant(nd_delta=0, skip=8):
    """qgram_ref.block_count (b = 8) with `nd_delta` more text dwords counted (the text behind a sequence is zero = 'A') and a counted gram
    covering `skip` bases"""
    def count(owner, partner, s):
        grams = set(owner[i:i + 8] for i in range(len(owner) - 7))
        nd = max(0, F.dwords(len(partner), s) + nd_delta)
        text = partner + "A" * 40
        cnt, nxt = 0, 0
        for p in range(0, 16 * nd, s):
            if p >= nxt and text[p:p + 8] not in grams:
                cnt += 1
                nxt = p + skip
        return cnt
    return count


def _owner_ignored(word, thr, owner, kcap):
    k = -1
    if word & F.OWNER_BIT:
        k = int(thr[owner])
    if word & F.PARTNER_BIT:
        k = int(thr[word & F.INDEX_MASK])
    return min(k, kcap)


def _no_kcap(word, thr, owner, kcap):
    return F.pair_threshold(word, thr, owner, 1 << 30)


# mutation -> (the changed piece of expect(), a designed case that must notice)
MUTATIONS = {
    "< for <=": (dict(le=operator.lt), "edge_k/partner"),
    "owner's threshold ignored when bit 31 is set": (dict(pair_threshold=_owner_ignored), "edge_k/owner"),
    "kcap not applied": (dict(pair_threshold=_no_kcap), "edge_k/kcap"),
    "last whole dword dropped": (dict(count=_count_variant(nd_delta=-1)), "lengths"),
    "one partial dword added": (dict(count=_count_variant(nd_delta=+1)), "lengths"),
    "skip behind a counted gram one probe short (stride 4)": (dict(count=lambda o, p, s: _count_variant(skip=8 - s)(o, p, s) if s == 4 else F.count(o, p, s)), "edge_k/partner"),
    "skip behind a counted gram one probe short (stride 2)": (dict(count=lambda o, p, s: _count_variant(skip=8 - s)(o, p, s) if s == 2 else F.count(o, p, s)), "edge_k/partner"),
    "2 np > count for >=": (dict(ge=operator.gt), "routing"),
    "15 for 16": (dict(pass2_min=15), "routing"),
}


def _same(a, b):
    return all(a[k] == b[k] for k in a if k != "per_chunk")


def test_the_variant_count_is_the_restatement():
    call = F.cases()["lengths"]
    same = _count_variant()
    for o, _, words in call.chunks[:4]:
        for w in words:
            for s in (4, 2):
                assert same(call.seqs[o], call.seqs[int(w) & F.INDEX_MASK], s) == qgram_ref.block_count(call.seqs[o], call.seqs[int(w) & F.INDEX_MASK], s=s)


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_wrong_rule_changes_the_answer(mutation):
    """what a kernel with this mistake would compute differs from expect() on the case designed for it (and the list of all cases that notice is printed)"""
    pieces, designed = MUTATIONS[mutation]
    caught = [(name, second) for name, call in F.cases().items() if name != "queue" for second in (1, 0) if not _same(F.expect(call, second, **pieces), F.expected(name, second))]
    print("%s: %s" % (mutation, ", ".join("%s/%d" % c for c in caught)))
    assert designed in [name for name, _ in caught], caught
