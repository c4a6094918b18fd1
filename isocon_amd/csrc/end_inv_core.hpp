// end_inv_core.hpp -- the pair rule of the end-invariant collapse (isocon_end_invariant_graph, end_inv.hpp) on the 2-bit planes: the test
// of get_invariants_under_ignored_edge_ends_speed (modules/end_invariant_functions.py:920-951 of the reference) with is_overlap (:884-918)
// for an ordered pair of the length-sorted store, A (length m, position i) and B (length n, position p).  The host statements of the same
// test: end_invariant_functions._pair_is_invariant and cpy/_pyhelp.c invariant_partners / overlap_holds.
//
// Window of row i (:934-936, :951): the positions lo <= p < hi, p != i, lo = first length >= m - 2 thr, hi = first length > m -- so
// n <= m, and equal lengths are visited from both sides.
//
// match(d): A[t + d] == B[t] for every t with 0 <= t < n and 0 <= t + d < m (the two coincide on their whole overlap under the shift d).
// With n > thr (the entry refuses shorter sequences: the "always true" branches of is_overlap stay on the host) the reference's test is
//   containment (:938-943, `seq2 in seq1`, `seq1.find(seq2)`): d* = the smallest d in [0, m - n] with match(d).  If there is one the pair
//     is invariant iff d* <= thr and m - n - d* <= thr, and nothing else is tried: the FIRST occurrence decides;
//   overlap (:945-950), otherwise: invariant iff match(d) for some d in (m - n, thr] -- is_overlap(seq1, seq2): the suffix of A of length
//     L = m - d equals a prefix of B, and m - L, n - L <= thr (:908-910; L < n because B is not contained at m - n) -- or for some d in
//     [m - n - thr, -1] -- is_overlap(seq2, seq1): the suffix of B of length L = n + d equals a prefix of A.  The reference looks for the
//     LONGEST such L and compares its two offsets; "some L within the threshold" is the same statement.
// The shifts to test are therefore d_lo .. thr with d_lo = min(0, m - n - thr): where m - n >= thr there is no overlap shift and a first
// occurrence beyond thr fails like none at all, where m - n < thr the whole of [0, m - n] is inside.  At most 2 thr + 1 shifts.
//
// A pair's verdict is the minimum of a key over its matching shifts (einv_key): a containment shift d is its own key, an overlap shift
// is EINV_KEY_OVERLAP, above every containment key; no match leaves EINV_KEY_NONE.  The minimum does not depend on the order in which
// the shifts are verified, which is what lets the device verify them one lane per (pair, shift).
//
// On the planes (common.hpp: planes[((chunk * n) + id) * 2 + plane], bases past the end 0, nchunks = ceil(maxlen / 64) + 1): the 64
// bases from position pos are a funnel of two adjacent words (einv_fetch); the difference word of two such reads is
// (a0 ^ b0) | (a1 ^ b1), masked to the bases of the overlap -- bases past a sequence's end read as code 0, which is 'A', so the mask
// comes from the lengths and never from the padding.  einv_fetch never indexes a chunk outside [0, nchunks): such a word is 0.
// The same header is compiled by g++ for tests/emul/end_inv_emul.cpp (CPU test of the rule against _pair_is_invariant, also under
// -fsanitize=undefined,address on a plane array of exactly nchunks * n * 2 words).
#pragma once
#include "hw_graph_core.hpp"

namespace isocon {

static constexpr int32_t EINV_MAX_THR = 1024;          // a pair costs up to 2 thr + 1 first-word tests
static constexpr uint32_t EINV_KEY_OVERLAP = 0x40000000u, EINV_KEY_NONE = 0xffffffffu;

// row i's window [lo, hi): lo <= i < hi
ISO_HD void einv_window(const int32_t *lens, uint32_t n, uint32_t i, int32_t thr, uint32_t &lo, uint32_t &hi)
{
    const int64_t m = lens[i];
    lo = hwg_lower(lens, n, m - 2 * (int64_t)thr);
    hi = hwg_upper(lens, n, m);
}

// the partner in slot r of row i (ascending positions, i itself left out)
ISO_HD uint32_t einv_slot_partner(uint32_t i, uint32_t lo, uint32_t r) { return lo + r + (lo + r >= i ? 1u : 0u); }

// the first shift to test (the last one is thr)
ISO_HD int32_t einv_first_shift(int32_t m, int32_t n, int32_t thr) { return m - n < thr ? m - n - thr : 0; }

// the overlap under shift d: B[t0 .. t0 + len) against A[t0 + d .. t0 + d + len); len > 0 for every shift tested when n > thr
ISO_HD void einv_overlap(int32_t m, int32_t n, int32_t d, int32_t &a0, int32_t &b0, int32_t &len)
{
    a0 = d > 0 ? d : 0;
    b0 = d < 0 ? -d : 0;
    const int32_t end = n < m - d ? n : m - d;
    len = end - b0;
}

// 64 bases of sequence `id` from position pos >= 0 on, one plane; a chunk outside the store reads as 0
ISO_HD uint64_t einv_fetch(const uint64_t *planes, uint32_t n, uint32_t nchunks, uint32_t id, uint32_t plane, int32_t pos)
{
    const uint32_t c = (uint32_t)pos >> 6, s = (uint32_t)pos & 63u;
    const uint64_t w0 = c < nchunks ? planes[((size_t)c * n + id) * 2 + plane] : 0ull;
    if (!s) return w0;
    const uint64_t w1 = c + 1u < nchunks ? planes[((size_t)(c + 1u) * n + id) * 2 + plane] : 0ull;
    return (w0 >> s) | (w1 << (64u - s));
}

// do two reads of 64 bases (planes a0 / a1 and b0 / b1) differ in their first `count` bases, 1 <= count <= 64
ISO_HD bool einv_words_differ(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, int32_t count)
{
    const uint64_t diff = (a0 ^ b0) | (a1 ^ b1);
    const uint64_t mask = count >= 64 ? ~0ull : (1ull << count) - 1ull;
    return (diff & mask) != 0ull;
}

// do A[apos .. apos + count) and B[bpos .. bpos + count) differ
ISO_HD bool einv_block_differs(const uint64_t *planes, uint32_t n, uint32_t nchunks, uint32_t a, uint32_t b, int32_t apos, int32_t bpos, int32_t count)
{
    return einv_words_differ(einv_fetch(planes, n, nchunks, a, 0, apos), einv_fetch(planes, n, nchunks, a, 1, apos),
                             einv_fetch(planes, n, nchunks, b, 0, bpos), einv_fetch(planes, n, nchunks, b, 1, bpos), count);
}

// the first 64 bases of a sequence: the side of the screen that does not move with the shift
struct EinvHead { uint64_t w0, w1; };
ISO_HD EinvHead einv_head(const uint64_t *planes, uint32_t n, uint32_t nchunks, uint32_t id)
{
    return EinvHead{einv_fetch(planes, n, nchunks, id, 0, 0), einv_fetch(planes, n, nchunks, id, 1, 0)};
}

// The screen: the first (up to) 64 bases of the overlap under shift d coincide.  One side of the overlap starts at its sequence's first
// base (B for d >= 0, A for d < 0), so a pair's shifts share the heads ha / hb and read one funnel each.
ISO_HD bool einv_first_word_matches(const uint64_t *planes, uint32_t n, uint32_t nchunks, uint32_t a, int32_t m, uint32_t b, int32_t nb, int32_t d,
                                    const EinvHead &ha, const EinvHead &hb)
{
    int32_t a0, b0, len;
    einv_overlap(m, nb, d, a0, b0, len);
    const int32_t count = len < 64 ? len : 64;
    if (d >= 0) return !einv_words_differ(einv_fetch(planes, n, nchunks, a, 0, a0), einv_fetch(planes, n, nchunks, a, 1, a0), hb.w0, hb.w1, count);
    return !einv_words_differ(ha.w0, ha.w1, einv_fetch(planes, n, nchunks, b, 0, b0), einv_fetch(planes, n, nchunks, b, 1, b0), count);
}

// match(d): the whole overlap, 64 bases at a time, until the first difference
ISO_HD bool einv_match(const uint64_t *planes, uint32_t n, uint32_t nchunks, uint32_t a, int32_t m, uint32_t b, int32_t nb, int32_t d)
{
    int32_t a0, b0, len;
    einv_overlap(m, nb, d, a0, b0, len);
    for (int32_t at = 0; at < len; at += 64)
        if (einv_block_differs(planes, n, nchunks, a, b, a0 + at, b0 + at, len - at < 64 ? len - at : 64)) return false;
    return true;
}

// the key of a matching shift
ISO_HD uint32_t einv_key(int32_t m, int32_t n, int32_t d) { return d >= 0 && d <= m - n ? (uint32_t)d : EINV_KEY_OVERLAP; }

// the verdict from the smallest key of the pair's matching shifts
ISO_HD bool einv_invariant(int32_t m, int32_t n, int32_t thr, uint32_t key)
{
    if (key == EINV_KEY_NONE) return false;
    if (key == EINV_KEY_OVERLAP) return true;
    return (int32_t)key <= thr && m - n - (int32_t)key <= thr;
}

// The rule for one pair, shift by shift (the emulator's loop; the kernels spread the same calls over lanes).  survivors / verified, if
// given, count the shifts that pass the screen and whether the pair had any.
ISO_HD bool einv_pair_invariant(const uint64_t *planes, uint32_t n, uint32_t nchunks, const int32_t *lens, uint32_t a, uint32_t b, int32_t thr,
                                uint64_t *survivors, uint64_t *verified)
{
    const int32_t m = lens[a], nb = lens[b];
    uint32_t key = EINV_KEY_NONE, seen = 0;
    const EinvHead ha = einv_head(planes, n, nchunks, a), hb = einv_head(planes, n, nchunks, b);
    for (int32_t d = einv_first_shift(m, nb, thr); d <= thr; ++d) {
        if (!einv_first_word_matches(planes, n, nchunks, a, m, b, nb, d, ha, hb)) continue;
        ++seen;
        if (einv_match(planes, n, nchunks, a, m, b, nb, d)) {
            const uint32_t k = einv_key(m, nb, d);
            key = k < key ? k : key;
        }
    }
    if (survivors) *survivors += seen;
    if (verified && seen) *verified += 1;
    return einv_invariant(m, nb, thr, key);
}

}  // namespace isocon
