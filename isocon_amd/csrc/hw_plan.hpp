// hw_plan.hpp -- what the host decides for the banded infix and prefix kernels (hw.hpp, hw_loc.hpp, shw.hpp) without a device: the greedy cut
// of a pair list into tiles of one query x up to 64 targets, its cut rules, and the LDS, column store and grid of k_hw_finish.  Plain C++ (no HIP):
// hw_host.inc runs it, tests/emul/hw_plan_emul.cpp drives it on its own (tests/test_hw_plan.py, also with -fsanitize=address,undefined).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "hw_core.hpp"

namespace isocon {

struct HwTiles {
    std::vector<uint32_t> tile_q[4], lane_pair[4];      // per class W = 1, 2, 4, 8
};

// Cut rules.  words(p) = window words of the band pair p needs on its own; fits(p, dmax, kmax, W) = does p still fit W words next to
// lanes whose largest length difference and largest threshold are dmax and kmax -- if so, these become the extremes with p.
struct HwLocateCut {          // hw_locate_rows(delta, thr) diagonals: LOCATE (thr = k) and ENDS (thr = the pair's distance)
    const int32_t *lens;
    const uint32_t *q, *t;
    const int32_t *thr;
    int32_t delta(uint32_t p) const { return lens[t[p]] - lens[q[p]]; }
    int words(uint32_t p) const { return hwt_words(hw_locate_rows(delta(p), thr[p])); }
    bool fits(uint32_t p, int32_t &dmax, int32_t &kmax, int W) const
    {
        const int32_t d2 = std::max(dmax, delta(p)), k2 = std::max(kmax, thr[p]);
        if (hw_locate_rows(d2, k2) > 64 * W) return false;
        dmax = d2; kmax = k2;
        return true;
    }
};
struct HwFinishCut {          // 2 k + 1 diagonals: START + TRACE of the hits
    const int32_t *k;
    int words(uint32_t p) const { return hwt_words(2 * k[p] + 1); }
    bool fits(uint32_t p, int32_t &dmax, int32_t &kmax, int W) const
    {
        const int32_t k2 = std::max(kmax, k[p]);
        if (2 * k2 + 1 > 64 * W) return false;
        dmax = 0; kmax = k2;
        return true;
    }
};
struct HwPrefixCut {          // 2 thr + 1 diagonals: the prefix passes (shw.hpp), thr = the round's threshold or the pair's distance
    const int32_t *thr;
    int words(uint32_t p) const { return thr[p] <= 255 ? hwt_words(2 * thr[p] + 1) : 0; }
    bool fits(uint32_t p, int32_t &dmax, int32_t &kmax, int W) const
    {
        const int32_t k2 = std::max(kmax, thr[p]);          // (the class of the largest threshold: joining a tile never widens it)
        if (2 * k2 + 1 > 64 * W) return false;
        dmax = 0; kmax = k2;
        return true;
    }
};

// Tiles of the pairs `idx` (any order): pairs are grouped by (words needed, query) with two counting sorts, a group is cut
// into tiles of at most 64 lanes whose COMMON window (largest length difference and largest threshold of the tile) still
// fits the class.  Empty lanes (0xffffffff) only at a tile's tail.
template <class Rule>
void hw_build_tiles(const std::vector<uint32_t> &idx, const uint32_t *q, uint32_t nseq, const Rule &rule, HwTiles &out)
{
    // stable counting sort by query, then a stable split by class
    std::vector<uint32_t> first((size_t)nseq + 1, 0);
    for (uint32_t p : idx) ++first[(size_t)q[p] + 1];
    for (uint32_t i = 0; i < nseq; ++i) first[i + 1] += first[i];
    std::vector<uint32_t> byq(idx.size());
    for (uint32_t p : idx) byq[first[q[p]]++] = p;
    for (int c = 0; c < 4; ++c) {
        const int Wc = 1 << c;
        std::vector<uint32_t> &tq = out.tile_q[c], &lp = out.lane_pair[c];
        uint32_t cur_q = 0xffffffffu;
        int32_t dmax = 0, kmax = 0;
        size_t fill = 64;
        for (uint32_t p : byq) {
            if (rule.words(p) != Wc) continue;
            int32_t d2 = dmax, k2 = kmax;
            const bool same = q[p] == cur_q && fill < 64 && rule.fits(p, d2, k2, Wc);
            if (!same) {
                while (fill < 64 && !tq.empty()) { lp.push_back(0xffffffffu); ++fill; }
                tq.push_back(q[p]);
                cur_q = q[p];
                fill = 0;
                d2 = -(1 << 30); k2 = 0;
                rule.fits(p, d2, k2, Wc);
            }
            dmax = d2; kmax = k2;
            lp.push_back(p);
            ++fill;
        }
        while (fill < 64 && !tq.empty()) { lp.push_back(0xffffffffu); ++fill; }
    }
}

// k_hw_finish<1|2> keeps checkpoints of the band state (every HW_SEG-th column) in its per-workgroup store and walks on segments
// recomputed into LDS; the wider classes store every column.
inline size_t hw_finish_lds(int Wc) { return Wc == 2 ? (size_t)HW_SEG * 2 * Wc * 64 * 8 : 0; }          // (one word: the segment stays in registers)
inline uint64_t hw_finish_store_bytes(int Wc, uint32_t trace_cols)
{
    return Wc <= 2 ? ((uint64_t)trace_cols / HW_SEG + 2) * 2 * Wc * 64 * 8 : ((uint64_t)trace_cols + 1) * 2 * Wc * 64 * 8;
}
inline uint32_t hw_finish_grid_cap(int Wc) { return Wc == 2 ? (uint32_t)(256 * (160 * 1024 / (hw_finish_lds(Wc) + 256))) : 4096u; }

// Workgroups of a k_hw_finish launch: one wavefront per tile in flight, each with its own column store -- as many as 16 per CU, bounded
// by memory (12 GiB, and a third of the `free_bytes` the device reports).
inline uint32_t hw_finish_grid(uint32_t n_tiles, int Wc, uint32_t trace_cols, uint64_t free_bytes)
{
    const uint64_t budget = std::min<uint64_t>((uint64_t)12 << 30, free_bytes / 3);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_tiles, hw_finish_grid_cap(Wc)), budget / hw_finish_store_bytes(Wc, trace_cols)));
}

}  // namespace isocon
