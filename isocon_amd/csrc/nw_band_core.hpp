// nw_band_core.hpp -- lane-level math of the BANDED global alignment path kernels (nw_band.hpp, gfx950): the paths of nw_path_core.hpp
// for a pair whose distance ed is known, computed on the diagonals an optimal path can touch and nowhere else.
// Specification: orc_nw_path (oracle/isocon_oracle.c section 5), as for the un-banded kernels.
//
// Rows are query positions i (1..m), columns target positions j (1..n), d = m - n.  Every optimal path stays on the diagonals i - j of
// the CORRIDOR [min(0, d) - x, max(0, d) + x], x = (ed - |d|) / 2 (lane_emin, band_core.hpp): |d| + 2 x + 1 <= ed + 1 diagonals.  One lane
// takes one pair through a window of 64 W rows that slides one row per column (the column step of band_core.hpp): the window of column j
// covers the rows a0 + j .. a0 + j + 64 W - 1, i.e. the diagonals [a0, a0 + 64 W - 1]; the origin a0 <= 0 is placed so that they contain
// the corridor.  Rows <= 0 are the virtual rows of band_init, which make the global top row D[0][j] = j come out without a special case.
//
// Per column the pass hands a sink, word by word,
//   vp   the vertical +1 vector AFTER the slide: bit r <-> D[a0 + j + 1 + r][j] - D[a0 + j + r][j] == +1
//   hp   the horizontal +1 vector of the column:  bit r <-> D[a0 + j + r][j] - D[a0 + j + r][j - 1] == +1
// and the value on the final diagonal after the last column is D[m][n], which must equal ed.
//
// The walk from (m, n) follows the oracle's rule (vertical +1: 'I', else horizontal +1: 'D', else the diagonal) on those vectors: the cell
// (i, j) is window bit b = i - j - a0 of column j, its vertical bit is vp bit b - 1 and its horizontal bit hp bit b.  A step whose
// destination lies outside the window is not taken -- the vertical step out of the window's first row (b = 0) and the horizontal step out
// of its last (b = 64 W - 1) read as 0.  That reproduces the full-matrix walk exactly: a cell the walk stands on lies on an optimal path,
// so its banded value is exact; a neighbour whose true delta is +1 lies on an optimal path too, hence inside the corridor and exact; any
// other neighbour has a banded value >= its true one, so its delta cannot read +1.  Along the borders the walk goes on as nwp_walk does.
// The same header is compiled by g++ for tests/emul/nw_band_emul.cpp.
#pragma once
#include "ed_lanes_core.hpp"
#include "nw_path_core.hpp"

namespace isocon {

static constexpr int32_t NWB_MAX_DIAGS = 256;      // the widest window: W = 4

// Number of diagonals of the corridor of a pair with d = m - n and distance ed (>= |d|).
ISO_HD int32_t nwb_corridor(int32_t d, int32_t ed)
{
    const int32_t ad = d < 0 ? -d : d;
    return ad + 2 * ((ed - ad) / 2) + 1;
}

// The smallest W of {1, 2, 4} whose window holds the corridor; 0: none does (or ed < |d|: no such pair), the pair is not banded.
ISO_HD int32_t nwb_class(int32_t d, int32_t ed)
{
    const int32_t ad = d < 0 ? -d : d;
    if (ed < ad) return 0;
    const int32_t c = nwb_corridor(d, ed);
    return c <= 64 ? 1 : c <= 128 ? 2 : c <= NWB_MAX_DIAGS ? 4 : 0;
}

// The window origin: the corridor's first diagonal on the window's first (the kernels' placement, no margin needed), or -- `last` --
// the corridor's last diagonal on the window's last (tests).  Both are <= 0.
ISO_HD int32_t nwb_origin(int32_t d, int32_t ed, int32_t W, bool last = false)
{
    const int32_t emin = lane_emin(d, ed);
    return last ? emin + nwb_corridor(d, ed) - 64 * W : emin;
}

// One column.  PL / PH: the complemented planes of the query positions [o, o + 64 W + 32) of the block, V: which of them are inside
// [0, m) (MASKED only); the window of the block's column jj is their bits jj .. jj + 64 W - 1.  wl / wh: the block's 32 text bases.
template <int W, bool MASKED, class Sink>
ISO_HD void nwb_column(BandLane<W> &L, const uint32_t (&PL)[2 * W + 1], const uint32_t (&PH)[2 * W + 1], const uint32_t (&V)[2 * W + 1], int jj,
                       uint32_t wl, uint32_t wh, int32_t col, Sink sink)
{
    const uint32_t sl = splat_bit(wl, jj), sh = splat_bit(wh, jj);
    uint64_t EQ[W], HP[W];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < W; ++i) {
        uint32_t e[2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * i + h;
            const uint32_t nl = funnel32(PL[k + 1], PL[k], jj), nh = funnel32(PH[k + 1], PH[k], jj);
#if defined(__HIP_DEVICE_COMPILE__)
            e[h] = __builtin_amdgcn_bitop3_b32(nl ^ sl, nh, sh, 0x60);          // (nl ^ sl) & (nh ^ sh)
#else
            e[h] = (nl ^ sl) & (nh ^ sh);
#endif
            if (MASKED) e[h] &= funnel32(V[k + 1], V[k], jj);
        }
        EQ[i] = ((uint64_t)e[1] << 32) | e[0];
    }
    band_step_eq_hp<W>(L, EQ, HP);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < W; ++i) sink(col, i, L.VP[i], HP[i]);
}

// The forward pass of one lane: query (m rows) against n columns through the window of origin a0.
//   qw(plane, p) / tw(plane, p)   32 bits of the query's / the text's bit-plane from position p on (p may be negative or run past the
//                                 end: zeros there); the text is the target, or its window (tw adds the window's start)
//   sink(col, word, vp, hp)       column col (0-based), see above; called for the columns below n, and -- on the device, where a wave's
//                                 lanes go through a block together -- possibly for later ones of the wave's longest lane
//   run                           this lane has a pair (m > 0, n > 0, the corridor inside the window); any: a vote of the wave
// Words for block c0 + 32 are requested before the columns of block c0 are computed.  Returns D[m][n] (-1 for a lane without a pair).
template <int W, class QW, class TW, class Sink, class Any>
ISO_HD int32_t nwb_forward(QW qw, TW tw, int32_t m, int32_t n, int32_t a0, bool run, Sink sink, Any any)
{
    constexpr int R = 2 * W + 1;
    const int32_t nv = -a0;
    BandLane<W> L;
    band_init<W>(L, nv, (m - n) - a0);
    int32_t r = -1, o = -nv;
    uint32_t PL[R], PH[R], V[R];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < R; ++k) { PL[k] = ~qw(0, o + 32 * k); PH[k] = ~qw(1, o + 32 * k); V[k] = 0; }
    uint32_t wl = tw(0, 0), wh = tw(1, 0);
    for (int32_t c0 = 0;; c0 += 32) {
        if (!any(run)) break;
        const uint32_t nwl = tw(0, c0 + 32), nwh = tw(1, c0 + 32);                      // the next block's words, in flight during this one
        const uint32_t nql = ~qw(0, o + 32 * R), nqh = ~qw(1, o + 32 * R);
        const bool full = c0 + 32 <= n;
        if (!any(run && (o < 0 || !full))) {
            // no virtual rows in any window of the block, 32 columns for every running lane
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
            for (int jj = 0; jj < 32; ++jj) nwb_column<W, false>(L, PL, PH, V, jj, wl, wh, c0 + jj, sink);
        } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < R; ++k) V[k] = lane_valid32(o + 32 * k, m);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int jj = 0; jj < 32; ++jj)
                if (run && c0 + jj < n) nwb_column<W, true>(L, PL, PH, V, jj, wl, wh, c0 + jj, sink);
        }
        if (run && c0 + 32 >= n) { r = band_diag_value<W>(L, nv, n); run = false; }
        o += 32;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k + 1 < R; ++k) { PL[k] = PL[k + 1]; PH[k] = PH[k + 1]; }
        PL[R - 1] = nql; PH[R - 1] = nqh;
        wl = nwl; wh = nwh;
    }
    return r;
}

// The walk from (m, n) to (0, 0) on what the pass kept.
//   load(i, j, word, vp, hp)   the unit of column j (1-based) and that word, for the cell (i, j): called once per step, by every lane
//                              that still walks (the one place where an implementation can fetch ahead for the whole wave)
//   side(j, word, vp, hp)      the same unit for the one bit that lies in the word below (b - 1 at a word's first bit)
//   same_base(i, j)            q[i - 1] == t[j - 1], for the (i, j) of the last load
//   emit(code, len)         one maximal run, in walk order = reversed
// Returns the number of runs, or -5 if the walk left the window (it cannot where the pass' score was the pair's distance).
template <int W, class Load, class Side, class Same, class Emit>
ISO_HD int32_t nwb_walk(int32_t m, int32_t n, int32_t a0, Load load, Side side, Same same_base, Emit emit)
{
    int32_t i = m, j = n, code = -1, len = 0, runs = 0;
    while (i > 0 && j > 0) {
        const int32_t b = i - j - a0;
        if (b < 0 || b >= 64 * W) return -5;
        uint64_t vp, hp;
        load(i, j, b >> 6, vp, hp);
        bool pv = false;
        if (b >= 1) {
            const int32_t bb = b - 1;
            if ((bb >> 6) == (b >> 6)) pv = (vp >> (bb & 63)) & 1;
            else { uint64_t v2, h2; side(j, bb >> 6, v2, h2); pv = (v2 >> 63) & 1; }
        }
        const bool ph = b < 64 * W - 1 && ((hp >> (b & 63)) & 1);
        int32_t c;
        if (pv) { c = NWP_I; --i; }
        else if (ph) { c = NWP_D; --j; }
        else { c = same_base(i, j) ? NWP_EQ : NWP_X; --i; --j; }
        if (c == code) ++len;
        else {
            if (len) { emit(code, len); ++runs; }
            code = c; len = 1;
        }
    }
    // the borders, as nwp_walk: 'I' down column 0, 'D' along row 0
    const int32_t c = i > 0 ? NWP_I : NWP_D, rest = i > 0 ? i : j;
    if (rest > 0) {
        if (c == code) len += rest;
        else {
            if (len) { emit(code, len); ++runs; }
            code = c; len = rest;
        }
    }
    if (len) { emit(code, len); ++runs; }
    return runs;
}

}  // namespace isocon
