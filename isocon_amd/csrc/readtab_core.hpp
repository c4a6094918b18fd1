// readtab_core.hpp -- lane-level math of the device read tables of the statistical test (readtab.hpp), shared with the CPU emulator
// of tests/emul (g++, also under UBSan).
//
// A row is one stored read alignment: the candidate's gapped row A and the read's gapped row B, equally long, over ACGT-.  Per block of
// 64 columns the table keeps
//     nob   bit c set: column c holds NO candidate base (A is '-' there, or the column lies past the row's end),
//     diff  bit c set: A and B differ in column c (0 past the end),
//     pre   candidate bases of A in the blocks before this one,
// and the bytes of B.  A table set with base qualities attached (isocon_readtab_set_qualities) also keeps
//     rgap  bit c set: B is '-' in column c (0 past the end),
//     rpre  read bases of B in the blocks before this one,
// from which the number of read bases up to a column -- and with it the place of a variant in the read's quality record -- follows.  What the per-read statements of the reference compute from the strings
// (modules/functions.py:149-201 get_support, :495-522 read_errors_from_alignment) becomes:
//     column of candidate base i      block b = the last one with pre[b] <= i, then the (i - pre[b])-th zero bit of nob[b]
//     aln_read[lo:hi] == aln_c[lo:hi]  no bit of diff in the columns [lo, hi)
//     errors between the end gaps      popcounts of the masks over [start, stop), start / stop from the end runs of both rows
// Every shift here is by 0 .. 63: a mask of 64 columns, a window that ends at bit 63 and a select in a full or empty word take the
// branches written out below.
#pragma once
#include "band_core.hpp"

namespace isocon {

// the n lowest bits, n in [0, 64]
ISO_HD uint64_t rt_low_mask(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : ((1ull << n) - 1ull); }

// Position of the n-th (0-based) ZERO bit of mask; 64 if mask has no more than n zero bits (a full word, n too large).
ISO_HD int rt_select_zero(uint64_t mask, int n)
{
    uint64_t z = ~mask;
    if (n < 0 || n >= popc64(z)) return 64;
    int pos = 0;
    for (int w = 32; w >= 1; w >>= 1) {          // halving: is the wanted bit among the low w bits of what is left?
        const int c = popc64(z & rt_low_mask(w));
        if (n >= c) { n -= c; z >>= w; pos += w; }
    }
    return pos;
}

// The last block b in [0, nb) with pre[b] <= i (pre ascends, pre[0] = 0, i >= 0); nb = 0 returns 0.  Blocks without a candidate base
// share their successor's count, so the block found holds base i whenever the row has more than i bases.
ISO_HD uint32_t rt_find_block(const uint32_t *pre, uint32_t nb, uint32_t i)
{
    uint32_t lo = 0, hi = nb;          // invariant: pre[lo] <= i, and pre[hi] > i or hi == nb
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pre[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// n bits (n in [0, 64]) from bit sh (in [0, 63]) of the 128-bit value w1:w0
ISO_HD uint64_t rt_window(uint64_t w0, uint64_t w1, int sh, int n)
{
    uint64_t v = w0 >> sh;
    if (sh) v |= w1 << (64 - sh);
    return v & rt_low_mask(n);
}

// the columns of block b (64 b .. 64 b + 63) that lie in [lo, hi), as a mask
ISO_HD uint64_t rt_range_mask(int64_t b, int64_t lo, int64_t hi)
{
    const int64_t c0 = b * 64;
    const int64_t a = lo > c0 ? lo - c0 : 0, e = hi - c0 < 64 ? hi - c0 : 64;
    if (e <= a) return 0ull;
    return rt_low_mask((int)e) & ~rt_low_mask((int)a);
}

// length of the run of set bits at the low / high end of the n valid (low) bits of a word, n in [0, 64]
ISO_HD int rt_lead_ones(uint64_t m, int n)
{
    const uint64_t z = ~m & rt_low_mask(n);
    return z ? __builtin_ctzll(z) : n;
}
ISO_HD int rt_trail_ones(uint64_t m, int n)
{
    const uint64_t z = ~m & rt_low_mask(n);
    return z ? n - 64 + __builtin_clzll(z) : n;
}

// The end runs of a gap mask taken block by block (blocks in ascending order): lead = gaps the row starts with, trail = gaps it ends with.
struct RtRuns {
    int64_t lead, trail, seen;
    bool in_lead;
};
ISO_HD RtRuns rt_runs_init() { return RtRuns{0, 0, 0, true}; }
ISO_HD void rt_runs_step(RtRuns &r, uint64_t gap, int n)
{
    if (r.in_lead) {
        const int l = rt_lead_ones(gap, n);
        r.lead += l;
        if (l < n) r.in_lead = false;
    }
    const int t = rt_trail_ones(gap, n);
    r.trail = t == n ? r.trail + t : t;
    r.seen += n;
}

// (insertions, deletions, substitutions) of one block inside [start, stop): a differing column counts as an insertion where A is a
// gap, else as a deletion where B is one, else as a substitution -- the if / elif / else of read_errors_from_alignment.
ISO_HD void rt_block_errors(uint64_t gap_a, uint64_t gap_b, uint64_t diff, int64_t b, int64_t start, int64_t stop, uint32_t &ins, uint32_t &dele, uint32_t &sub)
{
    const uint64_t d = diff & rt_range_mask(b, start, stop);
    ins += (uint32_t)popc64(d & gap_a);
    dele += (uint32_t)popc64(d & ~gap_a & gap_b);
    sub += (uint32_t)popc64(d & ~gap_a & ~gap_b);
}

// One row as the support queries see it.
struct RtRow {
    const uint64_t *nob;          // nb words
    const uint64_t *diff;         // nb words
    const uint32_t *pre;          // nb counts
    const uint8_t *read;          // len bytes of B
    uint32_t nb;
    int64_t len;
    const uint64_t *rgap = nullptr;          // nb words   } only with qualities attached (rt_read_bases_upto, rt_quality_code)
    const uint32_t *rpre = nullptr;          // nb counts  }
};

// column of candidate base i, 0 <= i < number of candidate bases of the row
ISO_HD int64_t rt_column_of(const RtRow &R, uint32_t i)
{
    const uint32_t b = rt_find_block(R.pre, R.nb, i);
    return (int64_t)b * 64 + rt_select_zero(R.nob[b], (int)(i - R.pre[b]));
}

// does a column of [lo, hi) differ?  (0 <= lo, hi <= len)
ISO_HD bool rt_any_diff(const RtRow &R, int64_t lo, int64_t hi)
{
    if (hi <= lo) return false;
    const int64_t b0 = lo >> 6, b1 = (hi - 1) >> 6;
    if (hi - lo <= 64)          // at most two words
        return rt_window(R.diff[b0], b1 > b0 ? R.diff[b1] : 0ull, (int)(lo & 63), (int)(hi - lo)) != 0;
    for (int64_t b = b0; b <= b1; ++b)
        if (R.diff[b] & rt_range_mask(b, lo, hi)) return true;
    return false;
}

// no differing column in [pos - 1, pos + u_v] within the row (pos: a column of the row)
ISO_HD bool rt_agrees_at(const RtRow &R, int64_t pos, int32_t u_v)
{
    const int64_t lo = pos - 1 > 0 ? pos - 1 : 0;
    int64_t hi = pos + (int64_t)u_v + 1;
    if (hi > R.len) hi = R.len;
    return !rt_any_diff(R, lo, hi);
}

// _ReadTable.agree_with_candidate for one variant: the window around the column of candidate base i
ISO_HD bool rt_agrees(const RtRow &R, uint32_t i, int32_t u_v) { return rt_agrees_at(R, rt_column_of(R, i), u_v); }

// the read's row shows the snippet in its (clipped) window around column pos: [pos - 2, pos + u_v) "insertion style", else [pos - 1, pos + u_v]
ISO_HD bool rt_shows_at(const RtRow &R, int64_t pos, int32_t u_v, bool is_insertion, const uint8_t *snippet, uint64_t snippet_len)
{
    const int64_t before = is_insertion ? 2 : 1, after = is_insertion ? (int64_t)u_v : (int64_t)u_v + 1;
    const int64_t lo = pos - before > 0 ? pos - before : 0;
    const int64_t hi = pos + after < R.len ? pos + after : R.len;
    const int64_t width = hi > lo ? hi - lo : 0;
    if ((uint64_t)width != snippet_len) return false;
    for (int64_t j = 0; j < width; ++j)
        if (R.read[lo + j] != snippet[j]) return false;
    return true;
}

// _ReadTable.show_snippets for one variant
ISO_HD bool rt_shows(const RtRow &R, uint32_t i, int32_t u_v, bool is_insertion, const uint8_t *snippet, uint64_t snippet_len)
{
    return rt_shows_at(R, rt_column_of(R, i), u_v, is_insertion, snippet, snippet_len);
}

// ---- base qualities: functions._ccs_probabilities (reference modules/functions.py:240-433) up to the quality it looks up ----

// _ReadTable.read_bases_upto: read bases in aln_read[:pos + 1], 0 <= pos < len
ISO_HD int64_t rt_read_bases_upto(const RtRow &R, int64_t pos)
{
    const int64_t b = pos >> 6;
    return (int64_t)R.rpre[b] + popc64(~R.rgap[b] & rt_low_mask((int)(pos & 63) + 1));
}

// What one read says at one variant, as a byte: its quality 0 .. 93 at the variant, or why there is none.
enum : uint8_t {
    RT_Q_INDEX = 0xFC,            // the place lies outside the quality record (the per-read statement raises IndexError)
    RT_Q_BEYOND = 0xFD,           // ... more than one past its end (CCS.read_aln_to_ccs_coord exits)
    RT_Q_BOTH = 0xFE,             // the read shows its own sequence AND the other one (the per-read statement asserts)
    RT_Q_NEITHER = 0xFF           // the read shows neither: not informative
};

// kind 0: a read of c judged against t (the shifted variant type is 'D'), kind 1: a read of t against c ('I').  qual: the read's
// record of rec_len qualities, the read starts at rec_start in it.  Both > neither > beyond > index > the quality.
ISO_HD uint8_t rt_quality_code(const RtRow &R, uint32_t i, int32_t u_v, uint8_t v_type, int kind, const uint8_t *snippet, uint64_t snippet_len, const uint8_t *qual,
                               int64_t rec_len, int64_t rec_start)
{
    const int64_t pos = rt_column_of(R, i);
    const bool shows_own = rt_agrees_at(R, pos, u_v);
    const bool shows_other = rt_shows_at(R, pos, u_v, v_type == (kind ? 'I' : 'D'), snippet, snippet_len);
    if (shows_own && shows_other) return RT_Q_BOTH;
    if (!shows_own && !shows_other) return RT_Q_NEITHER;
    const int64_t seen = rt_read_bases_upto(R, pos);
    int64_t off = -1;          // place of the judged base relative to the bases seen, for a read that shows the other sequence
    if (kind == 0 && v_type == 'I') off = 0;
    if (kind == 1 && v_type == 'D') off = 0;
    if (kind == 1 && v_type == 'I') off = -2;
    int64_t coord = rec_start + (shows_own ? seen - 1 : seen + off);          // CCS.read_aln_to_ccs_coord, then a Python list index
    if (coord > rec_len) return RT_Q_BEYOND;
    if (coord == rec_len) coord -= 1;
    if (coord < 0) coord += rec_len;
    if (coord < 0 || coord >= rec_len) return RT_Q_INDEX;
    return qual[coord];
}

// ---- the probabilities themselves: one read's share of one iteration of the variant loop of functions._ccs_probabilities ----

// A row's running state over the variants of a query.  p: the product so far while alive; -1.0 once a variant found the read not
// informative, -2.0 once it raised (alive is false from then on and later variants do nothing).
struct RtProb {
    double p;
    bool alive;
};
ISO_HD RtProb rt_prob_init() { return RtProb{1.0, true}; }

// what a step reports: nothing, or (variant index << 2 | rank) -- the smaller key is what the per-read statements meet first: variants
// in order, and within a variant the assertion on BOTH (rank 0) before the exit on BEYOND (1) before the IndexError (2)
constexpr uint32_t RT_P_NO_EVENT = 0xFFFFFFFFu;
constexpr uint32_t RT_P_MAX_VARIANTS = (1u << 24) - 2;          // (variant index + 1) << 8 fits a status word

// the status word of a query from the smallest key of its rows: 0 = no event, else (variant index + 1) << 8 | the code byte
ISO_HD uint32_t rt_prob_status(uint32_t key) { return key == RT_P_NO_EVENT ? 0u : ((((key >> 2) + 1u) << 8) | (uint32_t)(RT_Q_BOTH - (key & 3u))); }

// The step on a code byte.  ratios: substitution, insertion, deletion share of the edge's errors; p_of_quality: 94 error probabilities.
// binary64 multiplications and divisions in the association of the reference, never contracted, no reciprocal: the product is the
// reference's to the last bit, subnormal results included.
ISO_HD uint32_t rt_probability_apply(RtProb &s, uint8_t code, uint32_t v_index, int32_t u_v, uint8_t v_type, const double *ratios, const double *p_of_quality)
{
#pragma clang fp contract(off)
    if (!s.alive) return RT_P_NO_EVENT;
    if (code == RT_Q_NEITHER) {
        s = RtProb{-1.0, false};
        return RT_P_NO_EVENT;
    }
    if (code > 93) {          // BOTH, BEYOND or INDEX on a read that is still informative
        s = RtProb{-2.0, false};
        return (v_index << 2) | (uint32_t)(RT_Q_BOTH - code);
    }
    const double p10 = p_of_quality[code];
    double p_error;
    if (u_v > 1) p_error = p10;
    else if (v_type == 'S') p_error = (p10 * ratios[0]) / 3.0;
    else if (v_type == 'I') p_error = (p10 * ratios[1]) / 4.0;
    else p_error = p10 * ratios[2];
    s.p = s.p * p_error;
    return RT_P_NO_EVENT;
}

// One iteration for one read: rt_quality_code (same arguments), then the step above; v_index: the variant's place in its query.
ISO_HD uint32_t rt_probability_step(RtProb &s, uint32_t v_index, const double *ratios, const double *p_of_quality, const RtRow &R, uint32_t i, int32_t u_v, uint8_t v_type,
                                    int kind, const uint8_t *snippet, uint64_t snippet_len, const uint8_t *qual, int64_t rec_len, int64_t rec_start)
{
    if (!s.alive) return RT_P_NO_EVENT;          // (nothing is looked up for a read that has left)
    return rt_probability_apply(s, rt_quality_code(R, i, u_v, v_type, kind, snippet, snippet_len, qual, rec_len, rec_start), v_index, u_v, v_type, ratios, p_of_quality);
}

}  // namespace isocon
