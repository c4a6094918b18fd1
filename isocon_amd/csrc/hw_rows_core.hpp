// hw_rows_core.hpp -- lane-level math of the LANE-PER-PAIR un-banded infix ("HW") kernel (hw_rows.hpp, gfx950): the ends of the pairs
// whose band exceeds the 512 diagonals of hw_core.hpp and whose query has at most 64 W rows, W = 1, 2, 4 -- a primer, a barcode or an
// adapter against a whole read.  hw_full_core.hpp puts such a pair on a wavefront of which one lane works; here one lane IS one pair:
// the whole query sits in registers as W complemented plane words per plane and a row mask, the column step is the Myers / Hyyro block
// step of hwf_step over the W words of the column -- the horizontal delta leaving the 64th row of word w enters the first row of word
// w + 1, the carry between the words of band_core.hpp in the block form of hw_full_core.hpp --, the top row is free (horizontal input
// 0) and the value of the query's last row is tracked from the deltas at that row.  Lanes do not communicate.
//   count run: h = min over the columns of the last row, the first column attaining it, and how many columns attain the running
//              minimum (reset to 1 whenever the minimum improves)
//   fill run:  the same recurrence with h known: the caller takes every column whose last-row value equals h
// The same header is compiled by g++ for tests/emul/hw_rows_emul.cpp.
#pragma once
#include "hw_core.hpp"

namespace isocon {

template <int W>
struct HwrLane {
    uint64_t nlo[W], nhi[W], valid[W];   // the query's rows: complemented plane words, and which rows the query has
    uint64_t Pv[W], Mv[W];
    uint64_t last[W];                    // the bit of the query's last row (one bit in one word)
    int32_t score;                       // D[m][column just processed]
};

// smallest W of 1, 2, 4 whose 64 W rows hold a query of m bases (0: none does)
ISO_HD int hwr_words(int32_t m) { return m <= 0 ? 0 : (m <= 64 ? 1 : (m <= 128 ? 2 : (m <= 256 ? 4 : 0))); }

// lo(w) / hi(w): the two plane words of query rows 64 w + 1 .. 64 w + 64, m = query length (1 .. 64 W)
template <int W, class Lo, class Hi>
ISO_HD void hwr_init(HwrLane<W> &L, Lo lo, Hi hi, int32_t m)
{
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int32_t rem = m - 64 * w;
        L.nlo[w] = ~lo(w); L.nhi[w] = ~hi(w);
        L.valid[w] = rem <= 0 ? 0 : (rem >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << rem) - 1));
        L.last[w] = rem >= 1 && rem <= 64 ? (uint64_t)1 << (rem - 1) : 0;
        L.Pv[w] = ~(uint64_t)0; L.Mv[w] = 0;
    }
    L.score = m;
}

// One column: ch = the column's base.  Afterwards L.score = D[m][this column].
template <int W>
ISO_HD void hwr_step(HwrLane<W> &L, int32_t ch)
{
    const uint64_t sl = (uint64_t)0 - (uint64_t)(ch & 1), sh = (uint64_t)0 - (uint64_t)((ch >> 1) & 1);
    uint64_t hp = 0, hn = 0;             // the horizontal delta entering the word's first row: +1 / -1 (the top row: 0)
    uint64_t up = 0, dn = 0;             // the deltas at the query's last row
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint64_t Eq = (L.nlo[w] ^ sl) & (L.nhi[w] ^ sh) & L.valid[w];
        const uint64_t Pv = L.Pv[w], Mv = L.Mv[w];
        const uint64_t Xv = Eq | Mv;
        Eq |= hn;
        const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint64_t Ph = Mv | ~(Xh | Pv);
        uint64_t Mh = Pv & Xh;
        up |= Ph & L.last[w]; dn |= Mh & L.last[w];          // (any word may hold the last row: a query need not fill its instance)
        const uint64_t hp_out = Ph >> 63, hn_out = Mh >> 63;
        Ph = (Ph << 1) | hp;
        Mh = (Mh << 1) | hn;
        L.Pv[w] = Mh | ~(Xv | Ph);
        L.Mv[w] = Ph & Xv;
        hp = hp_out; hn = hn_out;
    }
    L.score += (int32_t)(up != 0) - (int32_t)(dn != 0);
}

// the count run's bookkeeping of one column (0-based col)
struct HwrCount {
    int32_t best, first;
    uint32_t count;
};
ISO_HD void hwr_count_init(HwrCount &c) { c.best = HWB_INF; c.first = -1; c.count = 0; }
ISO_HD void hwr_count_add(HwrCount &c, int32_t score, int32_t col)
{
    if (score < c.best) { c.best = score; c.first = col; c.count = 0; }
    c.count += (uint32_t)(score == c.best);
}

}  // namespace isocon
