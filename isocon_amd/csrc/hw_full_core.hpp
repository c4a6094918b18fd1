// hw_full_core.hpp -- lane-level math of the UN-BANDED infix ("HW") alignment kernels (hw_full.hpp, gfx950): the pairs whose band
// max(len_t - len_q, 0) + 2 k + 1 exceeds the 512 diagonals of hw_core.hpp.
//
// Same three passes and the same semantics as hw_core.hpp (specification: oracle/isocon_oracle.c section 5), but over the WHOLE query:
// one wavefront = one pair, lane l owns the 64 query rows of block 64 * pass + l (Myers / Hyyro block, vertical deltas Pv / Mv), the
// column loop is systolic -- at step s lane l works on column s - l, the horizontal delta of its last row and the text base travel one
// lane down per step.  Queries above 4 096 rows run in passes of 64 blocks; the horizontal deltas of the boundary row between two
// passes go through a buffer of 2 bits per column.
//   LOCATE  top row free (horizontal input 0), every column: h = min of the last row, end = the first column attaining it.
//   START   reversed query against the reversed prefix t[0..end], top-row delta +1: the LAST column of the last row equal to h.
//   TRACE   query against t[start..end], top-row delta +1; every column and block keeps its new Pv (bit r: the vertical step into row
//           r + 1 of the block is optimal) and its Ph (bit r: the horizontal step into that row is), the walk from the end cell prefers
//           the query-only step ('I'), then the target-only one ('D'), then the diagonal.
//   ENDS    the recurrence of LOCATE (top row free, every column) without its bookkeeping: the caller reads the last row's value after
//           every column (hw_rows.hpp: the columns attaining the distance are counted, then listed).
// The same header is compiled by g++ for tests/emul/hw_full_emul.cpp (64 emulated lanes in lock step, against the oracle).
#pragma once
#include "hw_core.hpp"

namespace isocon {

enum { HWF_LOCATE = 0, HWF_START = 1, HWF_TRACE = 2, HWF_ENDS = 3 };

struct HwfLane {
    uint64_t nlo, nhi, valid;          // the block's rows: complemented plane words, and which rows the query has
    uint64_t Pv, Mv;
    int32_t lastbit;                   // the block's last query row (63, or less in the query's last block)
    int32_t score;                     // D[that row][column just processed]
    int32_t best, best_col;            // LOCATE: minimum of score and the first 0-based column attaining it; START: the last column with score == h
};

ISO_HD int32_t hwf_blocks(int32_t m) { return (m + 63) >> 6; }
ISO_HD int32_t hwf_passes(int32_t m) { return (hwf_blocks(m) + 63) >> 6; }
ISO_HD int32_t hwf_pass_lanes(int32_t m, int32_t pass)
{
    const int32_t nb = hwf_blocks(m) - 64 * pass;
    return nb > 64 ? 64 : nb;
}

// lo / hi: the two plane words of query rows row0 + 1 .. row0 + 64 (forward or reversed stream), m = query length
ISO_HD void hwf_lane_init(HwfLane &L, uint64_t lo, uint64_t hi, int32_t m, int32_t row0)
{
    const int32_t rem = m - row0;
    const uint64_t vmask = rem <= 0 ? 0 : (rem >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << rem) - 1));
    L.nlo = ~lo; L.nhi = ~hi; L.valid = vmask;
    L.Pv = ~(uint64_t)0; L.Mv = 0;
    L.lastbit = (rem > 0 && rem < 64) ? rem - 1 : 63;
    L.score = row0 + L.lastbit + 1;
    L.best = HWB_INF; L.best_col = -1;
}

// One column of one block: ch = the column's base, hin = the horizontal delta entering the block's first row (-1, 0, +1), col = the
// 0-based column.  Returns the horizontal delta leaving the block's 64th row; ph = the "+1" horizontal deltas of the block's rows.
template <int MODE>
ISO_HD int32_t hwf_step(HwfLane &L, int32_t ch, int32_t hin, int32_t col, int32_t h, uint64_t &ph)
{
    // rows holding the column's base (as in hw_core.hpp: no table of four masks, which the compiler would index dynamically)
    const uint64_t sl = (uint64_t)0 - (uint64_t)(ch & 1), sh = (uint64_t)0 - (uint64_t)((ch >> 1) & 1);
    uint64_t Eq = (L.nlo ^ sl) & (L.nhi ^ sh) & L.valid;
    const uint64_t Pv = L.Pv, Mv = L.Mv;
    const uint64_t hneg = (uint64_t)(hin < 0);
    const uint64_t Xv = Eq | Mv;
    Eq |= hneg;
    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint64_t Ph = Mv | ~(Xh | Pv);
    uint64_t Mh = Pv & Xh;
    ph = Ph;
    const int32_t hout = (int32_t)(Ph >> 63) - (int32_t)(Mh >> 63);
    L.score += (int32_t)((Ph >> L.lastbit) & 1) - (int32_t)((Mh >> L.lastbit) & 1);
    Ph = (Ph << 1) | (uint64_t)(hin > 0);
    Mh = (Mh << 1) | hneg;
    L.Pv = Mh | ~(Xv | Ph);
    L.Mv = Ph & Xv;
    if (MODE == HWF_LOCATE) {
        if (L.score < L.best) { L.best = L.score; L.best_col = col; }
    } else if (MODE == HWF_START) {
        if (L.score == h) L.best_col = col;
    }
    return hout;
}

// what travels from lane l to lane l + 1: the column's base and the horizontal delta
ISO_HD int32_t hwf_pack(int32_t ch, int32_t hout) { return (ch << 2) | (hout + 1); }
ISO_HD int32_t hwf_packed_base(int32_t packed) { return packed >> 2; }
ISO_HD int32_t hwf_packed_delta(int32_t packed) { return (packed & 3) - 1; }

// boundary row between two passes: 2 bits per column, 16 columns per word.  The last lane of a pass collects a word in a register
// (hwf_bound_add) and writes it when its 16th column or the last column is done (hwf_bound_full); lane 0 of the next pass reads it.
ISO_HD uint32_t hwf_bound_words(int32_t ncols) { return (uint32_t)((ncols + 15) >> 4); }
ISO_HD uint32_t hwf_bound_add(uint32_t word, int32_t col, int32_t hout) { return word | ((uint32_t)(hout + 1) << ((col & 15) * 2)); }
ISO_HD bool hwf_bound_full(int32_t col, int32_t ncols) { return (col & 15) == 15 || col == ncols - 1; }
ISO_HD int32_t hwf_bound_get(uint32_t word, int32_t col) { return (int32_t)((word >> ((col & 15) * 2)) & 3u) - 1; }

// The TRACE store of one pair, in units of 16 bytes (one unit = one block's Pv and Ph of one column):
//   [0, hwf_fin_units)                    the LAST column's Pv of every block, 8 bytes each (the trailing insertion run is read off it)
//   then per pass (ms + lanes - 1) x lanes units, indexed [step][lane] -- what a wavefront writes in one step is one contiguous run of
//   16 * lanes bytes -- each pass rounded up to 512 bytes.  Every pass but the last has 64 lanes.
ISO_HD uint64_t hwf_round32(uint64_t units) { return (units + 31) & ~(uint64_t)31; }
ISO_HD uint64_t hwf_fin_units(int32_t m) { return hwf_round32(((uint64_t)hwf_blocks(m) + 1) >> 1); }
ISO_HD uint64_t hwf_pass_units(int32_t ms, int32_t lanes) { return hwf_round32(((uint64_t)ms + (uint64_t)lanes - 1) * (uint64_t)lanes); }
ISO_HD uint64_t hwf_pass_base(int32_t m, int32_t ms, int32_t pass) { return hwf_fin_units(m) + (uint64_t)pass * hwf_pass_units(ms, 64); }
ISO_HD uint64_t hwf_trace_units(int32_t m, int32_t ms)
{
    const int32_t last = hwf_passes(m) - 1;
    return hwf_pass_base(m, ms, last) + hwf_pass_units(ms, hwf_pass_lanes(m, last));
}
// unit of (block, 1-based column j)
ISO_HD uint64_t hwf_trace_unit(int32_t m, int32_t ms, int32_t block, int32_t j)
{
    const int32_t pass = block >> 6, lane = block & 63;
    return hwf_pass_base(m, ms, pass) + ((uint64_t)(j - 1) + (uint64_t)lane) * (uint64_t)hwf_pass_lanes(m, pass) + (uint64_t)lane;
}

ISO_HD int hwf_clz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The trailing insertion run: the consecutive optimal vertical steps at the end cell (m, ms).  fin(block) = the last column's Pv.
template <class Fin>
ISO_HD int32_t hwf_trail(int32_t m, Fin fin)
{
    int32_t t = 0, i = m;
    while (i > 0) {
        const int32_t bit = (i - 1) & 63;
        const uint64_t x = ~fin((i - 1) >> 6) << (63 - bit);          // bit 63 <-> row i, downwards; the shifted-in bits are zeros
        const int32_t run = x == 0 ? bit + 1 : hwf_clz64(x);
        t += run; i -= run;
        if (run < bit + 1) break;
    }
    return t;
}

// The walk of the TRACE pass from the end cell (m, ms).  load(block, j, pv, ph): what the pass kept for column j (1-based) of the block.
// Returns the leading insertion run: the rows left when column 0 is reached.
template <class Load>
ISO_HD int32_t hwf_walk(int32_t m, int32_t ms, Load load)
{
    int32_t i = m, j = ms;
    while (i > 0 && j > 0) {
        const int32_t bit = (i - 1) & 63;
        uint64_t pv, ph;
        load((i - 1) >> 6, j, pv, ph);
        if ((pv >> bit) & 1) --i;
        else if ((ph >> bit) & 1) --j;
        else { --i; --j; }
    }
    return j == 0 ? i : 0;
}

}  // namespace isocon
