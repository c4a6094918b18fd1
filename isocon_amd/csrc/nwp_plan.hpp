// nwp_plan.hpp -- what the host decides for the alignment path kernels (nw_path.hpp, nw_band.hpp) and the finish launches of the un-banded
// infix kernels (hw_full.hpp) without a device: the class of every hit and what its trace store needs, the two budgets and their refusals, the
// LDS bound, the order on the device, the slices of the reversed runs, the band waves, the greedy cut of hits and waves into launches, and
// the offsets of the forward ops.  Plain C++ (no HIP): nwp_paths (nw_path_host.inc) and hwf_pairs (hw_full_host.inc) run it,
// tests/emul/nwp_plan_emul.cpp drives it on its own (tests/test_nwp_plan.py, also with -fsanitize=address,undefined).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/isocon_hip.h"
#include "hw_full_core.hpp"
#include "nw_band_core.hpp"
#include "nw_path_core.hpp"

namespace isocon {

// Trace scratch one launch of k_nwp_trace may hold (SLOT_HW_TRACE, shared with the un-banded infix kernels): the host cuts the hits
// into as many launches as that takes, a pair whose own store exceeds it is refused.  The LDS limit of the boundary row is kHwfMaxLds.
static constexpr uint64_t kNwpTraceBudget = (uint64_t)1 << 30;
// The same for one launch of k_nwb_trace (nw_band.hpp, SLOT_NWB_TRACE), counted on the regions of its waves: a hit whose corridor fits
// 256 diagonals is traced there, on 16 bytes per column and window word.  A wave whose region exceeds the budget is cut into waves of
// fewer lanes, a pair whose own columns exceed it is refused.
static constexpr uint64_t kNwpBandBudget = (uint64_t)1 << 30;
// The same for one launch of k_hwf_finish (SLOT_HW_TRACE).
static constexpr uint64_t kHwfTraceBudget = (uint64_t)1 << 30;
static constexpr size_t kHwfMaxLds = (size_t)160 << 10;

// 16-byte units of the region of a band wave: [column][word][lane], the columns rounded up to the blocks of 32 the kernel works in
inline int32_t nwb_region_cols(int32_t cols) { return (cols + 31) & ~31; }
inline uint64_t nwb_region_units(int32_t cols, int32_t W, int32_t lanes) { return (uint64_t)nwb_region_cols(cols) * (uint64_t)W * (uint64_t)lanes; }

// Launches of consecutive items whose stores fit a budget together.  Launch c holds the items cut[c] .. cut[c + 1] - 1; off[i] is the
// store of item i in 16-byte units from the start of its launch's, most the largest store of a launch, sum that of all items.
struct BudgetCut {
    std::vector<size_t> cut = {0};
    std::vector<uint64_t> off;
    uint64_t most = 0, sum = 0;
    size_t launches() const { return cut.size() - 1; }
};

// An item joins the current launch unless that exceeds `budget` bytes, the launch holds `cap` items already, or new_launch(i) says so;
// a launch is never empty (an item above the budget -- the callers refuse it -- would be one of its own).
template <class NewLaunch>
inline BudgetCut budget_cut(const uint64_t *units, size_t n, uint64_t budget, size_t cap, NewLaunch new_launch)
{
    BudgetCut c;
    c.off.resize(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i > c.cut.back() && ((total + units[i]) * 16 > budget || i - c.cut.back() >= cap || new_launch(i))) { c.cut.push_back(i); total = 0; }
        c.off[i] = total; total += units[i];
        c.most = std::max(c.most, total);
        c.sum += units[i];
    }
    if (n) c.cut.push_back(n);
    return c;
}
inline BudgetCut budget_cut(const uint64_t *units, size_t n, uint64_t budget, size_t cap = (size_t)1 << 20)
{
    return budget_cut(units, n, budget, cap, [](size_t) { return false; });
}

// The pairs whose path is traced, in the order of the list.  start / cols: the window of the target of each (isocon_hw_path_pairs,
// isocon_shw_path_pairs); both empty: the whole target (isocon_ed_path_pairs).
struct NwpHits {
    std::vector<uint64_t> pair;
    std::vector<uint32_t> q, t;
    std::vector<int32_t> ed, start, cols;
    bool window() const { return !start.empty() || !cols.empty(); }
};

// Everything a path call knows before it touches the device.  On the device the un-banded hits come first, in the order of the list
// (positions 0 .. nu - 1), then the band hits by class and by number of columns (a wave's region is sized by its longest lane);
// ord[position] = hit.  A band wave is up to 64 consecutive positions of one class, the last of them the longest.
struct NwpPlan {
    std::vector<int32_t> cls, ncols;                  // by hit: class W (0: un-banded), columns
    std::vector<uint64_t> units_of;                   // by hit: 16-byte units of the un-banded store (0 for a band hit)
    double per_class[5] = {0, 0, 0, 0, 0};            // hits by W
    size_t nu = 0, lds = 0;                           // un-banded hits; LDS bytes of the boundary row of k_nwp_trace
    std::vector<uint32_t> ord, pq, pt;                // by position from here
    std::vector<int32_t> ped, pstart, pcols;
    std::vector<uint64_t> rev_off;                    // slices of the reversed runs: nwp_max_runs(ed) each
    uint64_t rev_total = 0;
    BudgetCut unbanded;                               // launches of positions 0 .. nu - 1; off: trace_off
    std::vector<uint32_t> slots;                      // by wave from here: 64 positions each, 0xffffffff at the tail
    std::vector<int32_t> wcols, wlanes, wcls;         // region columns, lanes, class
    BudgetCut band;                                   // launches of waves, one class each; off: wave_off
};

// lens: the store's lengths.  A refusal is its status and its sentence in `error` (the entry's name goes in front).
inline int nwp_plan(const std::vector<int32_t> &lens, const NwpHits &H, uint64_t budget, uint64_t band_budget, bool unbanded, NwpPlan &P, std::string &error,
                    size_t launch_cap = (size_t)1 << 20)
{
    const bool window = H.window();
    const size_t nh = H.pair.size();
    // ---- the class of every hit and what its store needs ----
    P.cls.assign(nh, 0); P.ncols.assign(nh, 0); P.units_of.assign(nh, 0);
    for (size_t i = 0; i < nh; ++i) {
        const int32_t m = lens[H.q[i]], nt = lens[H.t[i]], nc = window ? H.cols[i] : nt;
        if (window && (H.start[i] < 0 || nc <= 0 || nc > nt - H.start[i])) {
            error = "internal status (window) for pair " + std::to_string(H.pair[i]);
            return ISOCON_E_HIP;
        }
        P.ncols[i] = nc;
        if (!unbanded && m > 0 && nc > 0 && H.ed[i] >= 0) P.cls[i] = nwb_class(m - nc, H.ed[i]);
        const std::string sizes = "a query of " + std::to_string(m) + " bases against a target of " + std::to_string(nt) + " bases" +
                                  (window ? " (window of " + std::to_string(nc) + " columns)" : std::string());
        if (P.cls[i]) {
            const uint64_t need = nwb_region_units(nc, P.cls[i], 1) * 16;
            if (need > band_budget) {
                error = "the banded trace of " + sizes + " needs " + std::to_string(need) + " bytes (budget " + std::to_string(band_budget) + ")";
                return ISOCON_E_UNSUPPORTED;
            }
            P.per_class[P.cls[i]] += 1;
            continue;
        }
        const uint64_t u = hwf_trace_units(m, nc);
        if (u * 16 > budget) {
            error = "the trace of " + sizes + " needs " + std::to_string(u * 16) + " bytes (budget " + std::to_string(budget) + ")";
            return ISOCON_E_UNSUPPORTED;
        }
        if (hwf_passes(m) > 1) P.lds = std::max(P.lds, (size_t)hwf_bound_words(nc) * 4);
        P.units_of[i] = u;
        ++P.nu;
    }
    if (P.lds > kHwfMaxLds) {
        error = "a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
        return ISOCON_E_UNSUPPORTED;
    }
    // ---- the order on the device, and what is indexed by position ----
    const size_t nu = P.nu;
    const std::vector<int32_t> &cls = P.cls, &ncols = P.ncols;
    P.ord.resize(nh);
    {
        size_t a = 0, b = nu;
        for (size_t i = 0; i < nh; ++i) P.ord[cls[i] ? b++ : a++] = (uint32_t)i;
        std::sort(P.ord.begin() + nu, P.ord.end(), [&](uint32_t x, uint32_t y) {
            return cls[x] != cls[y] ? cls[x] < cls[y] : ncols[x] != ncols[y] ? ncols[x] < ncols[y] : x < y;
        });
    }
    P.pq.resize(nh); P.pt.resize(nh); P.ped.resize(nh); P.pstart.assign(nh, 0); P.pcols.resize(nh); P.rev_off.resize(nh);
    std::vector<int32_t> pcls(nh);
    std::vector<uint64_t> units(nh);
    for (size_t p = 0; p < nh; ++p) {
        const uint32_t i = P.ord[p];
        P.pq[p] = H.q[i]; P.pt[p] = H.t[i]; P.ped[p] = H.ed[i]; P.pcols[p] = ncols[i]; pcls[p] = cls[i]; units[p] = P.units_of[i];
        if (window) P.pstart[p] = H.start[i];
        P.rev_off[p] = P.rev_total;
        P.rev_total += nwp_max_runs(H.ed[i]);
    }
    // ---- the un-banded launches ----
    P.unbanded = budget_cut(units.data(), nu, budget, launch_cap);
    // ---- the band waves: a region above the budget is cut into waves of fewer lanes (every pair fits alone: checked above) ----
    std::vector<uint64_t> wunits;
    for (size_t p = nu; p < nh;) {
        const int32_t W = pcls[p];
        size_t e = p;
        while (e < nh && e - p < 64 && pcls[e] == W) ++e;
        if (nwb_region_units(P.pcols[e - 1], W, (int32_t)(e - p)) * 16 > band_budget) {
            const uint64_t per = std::max<uint64_t>(1, band_budget / (nwb_region_units(P.pcols[e - 1], W, 1) * 16));
            e = p + (size_t)std::min<uint64_t>(per, e - p);
        }
        const int32_t lanes = (int32_t)(e - p);          // a region has the lanes of its wave: 64 but for the last wave of a class
        P.slots.resize(P.slots.size() + 64, 0xffffffffu);
        for (int32_t l = 0; l < lanes; ++l) P.slots[P.slots.size() - 64 + l] = (uint32_t)(p + l);
        P.wcols.push_back(nwb_region_cols(P.pcols[e - 1])); P.wlanes.push_back(lanes); P.wcls.push_back(W);
        wunits.push_back(nwb_region_units(P.pcols[e - 1], W, lanes));
        p = e;
    }
    P.band = budget_cut(wunits.data(), wunits.size(), band_budget, launch_cap, [&](size_t w) { return P.wcls[w] != P.wcls[w - 1]; });
    return ISOCON_OK;
}

// Offsets of the dense forward list: a traced pair has its runs (by hit), another pair what extra(p) says.  out_ops_ptr[0 .. n_pairs];
// foff[position] = where the hit at that position starts.
template <class Extra>
inline void nwp_forward_offsets(const NwpHits &H, const std::vector<uint32_t> &ord, const std::vector<int32_t> &runs, uint64_t n_pairs, Extra extra,
                                uint64_t *out_ops_ptr, std::vector<uint64_t> &foff)
{
    const size_t nh = H.pair.size();
    size_t h = 0;
    uint64_t at = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        out_ops_ptr[p] = at;
        if (h < nh && H.pair[h] == p) at += (uint64_t)runs[h++];
        else at += extra(p);
    }
    out_ops_ptr[n_pairs] = at;
    foff.resize(nh);
    for (size_t p = 0; p < nh; ++p) foff[p] = out_ops_ptr[H.pair[ord[p]]];
}

}  // namespace isocon
