// hw_graph_core.hpp -- index arithmetic of the candidate-vs-candidate graph with ignored ends (isocon_hw_window_graph, hw_graph.hpp):
// which neighbours the loop of get_all_NN (modules/end_invariant_functions.py:622-681 of the reference) visits for an entry of the
// length-sorted list, in which order, and the end rules of edlib_traceback (:593-620) on a row of the infix kernels.
//
// The loop of entry i runs the offset j = 1, 2, ... with i - j before i + j; a side ends for good at the first length difference above
// `window` or at the list's end, and the offsets stop at jmax = max(1, min(depth, n)).  The lengths ascend, so the side below i holds
// the cd entries i - 1 .. i - cd and the side above it the cu entries i + 1 .. i + cu, and the visit order is a closed form of (cd, cu):
// the first 2 min(cd, cu) slots alternate down / up, then the longer side goes on alone.  Whether t is visited from i depends on
// |len_i - len_t| and |i - t| only, so i has a slot in the list of every t it visits: the "reverse slot".
// The same header is compiled by g++ for tests/emul/hw_graph_core_main.cpp (CPU test of these maps against the Python statement).
#pragma once
#include "band_core.hpp"

namespace isocon {

// first index whose length is >= v / > v (lens ascending)
ISO_HD uint32_t hwg_lower(const int32_t *lens, uint32_t n, int64_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)lens[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
ISO_HD uint32_t hwg_upper(const int32_t *lens, uint32_t n, int64_t v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)lens[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the largest offset of the loop (:677: the offsets stop at the depth, and the first one is always made)
ISO_HD uint32_t hwg_jmax(uint64_t depth, uint32_t n)
{
    const uint64_t d = depth < (uint64_t)n ? depth : (uint64_t)n;
    return d < 1 ? 1u : (uint32_t)d;
}

// neighbours of entry i below (cd) and above (cu) it
ISO_HD void hwg_counts(const int32_t *lens, uint32_t n, uint32_t i, int32_t window, uint32_t jmax, uint32_t &cd, uint32_t &cu)
{
    const int64_t li = lens[i];
    const uint32_t lo = hwg_lower(lens, n, li - window), hi = hwg_upper(lens, n, li + window);          // lo <= i < hi
    cd = i - lo < jmax ? i - lo : jmax;
    cu = hi - 1u - i < jmax ? hi - 1u - i : jmax;
}

// the neighbour in slot r < cd + cu of entry i
ISO_HD uint32_t hwg_slot_target(uint32_t i, uint32_t cd, uint32_t cu, uint32_t r)
{
    const uint32_t both = cd < cu ? cd : cu;
    if (r < 2u * both) {
        const uint32_t j = (r >> 1) + 1u;
        return (r & 1u) ? i + j : i - j;
    }
    const uint32_t j = r - both + 1u;          // both + (r - 2 both) + 1
    return cd > cu ? i - j : i + j;
}

// the slot of neighbour t in the list of entry i (t != i, within i's cd / cu)
ISO_HD uint32_t hwg_slot_of(uint32_t i, uint32_t cd, uint32_t cu, uint32_t t)
{
    const uint32_t both = cd < cu ? cd : cu;
    const bool down = t < i;
    const uint32_t j = down ? i - t : t - i;
    if (j <= both) return 2u * (j - 1u) + (down ? 0u : 1u);
    return both + j - 1u;                      // 2 both + (j - both - 1)
}

// _ends_adjusted / edlib_traceback (:597-619) on one row (distance, start, end, leading I run, trailing I run) with the target's length:
// target bases outside [start, end] beyond the threshold are charged, a terminal insertion run is forgiven up to the threshold.
// The value if the pair is a directed edge (distance >= 0 and 0 <= value <= max_ed), else -1.
ISO_HD int32_t hwg_edge_value(const int32_t *row, int32_t len_t, int32_t T, int32_t max_ed)
{
    if (row[0] < 0) return -1;
    const int64_t left = (int64_t)row[1] - T, right = (int64_t)len_t - ((int64_t)row[2] + 1) - T;
    const int64_t adj = (int64_t)row[0] + (left > 0 ? left : 0) + (right > 0 ? right : 0) - (row[4] < T ? row[4] : T) - (row[3] < T ? row[3] : T);
    return adj >= 0 && adj <= (int64_t)max_ed ? (int32_t)adj : -1;
}

}  // namespace isocon
