// end_inv.hpp -- the invariance graph of the end-invariant collapse built on the device (isocon_end_invariant_graph): device side of
// get_invariants_under_ignored_edge_ends_speed (modules/end_invariant_functions.py:920-951 of the reference, is_overlap :884-918).
// The rule, the window and the reads of the planes: end_inv_core.hpp.
//   k_einv_window  one thread per entry: the first position of its window and the number of its partners (two binary searches)
//   k_einv_screen  one thread per window pair, neighbouring lanes hold neighbouring partners (their plane words are adjacent in memory):
//                  every shift of the pair on the first 64 bases of its overlap; the surviving (pair, shift) are appended to one list
//                  (ballot, one atomic per wavefront and shift with a survivor)
//   k_einv_verify  one thread per survivor: the whole overlap, 64 bases at a time until the first difference; a match lowers the pair's
//                  key (atomicMin: the smallest containment shift, else "an overlap shift matched" -- independent of the list's order)
//   k_einv_rows    one wavefront per entry, a count pass and a write pass: the verdict from each partner's key, the invariant partners in
//                  ascending position (ballot compaction)
// No LDS; the only atomics are the list cursor, two counters and the per-pair minimum.
#pragma once
#include "common.hpp"
#include "end_inv_core.hpp"

namespace isocon {

// counters of one call (the first two are kept on the device, zeroed by the host)
enum { EINV_SURVIVORS = 0, EINV_VERIFIED, EINV_DEV_COUNTERS };
enum { EINV_OUT_PAIRS = 0, EINV_OUT_SURVIVORS, EINV_OUT_VERIFIED, EINV_OUT_INVARIANT, EINV_OUT_COUNTERS };

__global__ __launch_bounds__(256) void k_einv_window(const int32_t *__restrict__ lens, uint32_t n, int32_t thr, uint32_t *__restrict__ lo_out, uint32_t *__restrict__ tot_out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t lo, hi;
    einv_window(lens, n, i, thr, lo, hi);
    lo_out[i] = lo;
    tot_out[i] = hi - lo - 1u;
}

// the entry that owns slot p: the last one whose first slot is <= p (entries without a slot share their successor's first slot)
__device__ __forceinline__ uint32_t einv_owner(const unsigned long long *__restrict__ first, uint32_t n, unsigned long long p)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// first[i] = slots before entry i (first[n] = n_pairs).  surv: (slot, shift) records, room for surv_cap; the cursor ctr[EINV_SURVIVORS]
// counts on beyond it, so the host learns the room a second run needs.
__global__ __launch_bounds__(256) void k_einv_screen(DevStore S, const unsigned long long *__restrict__ first, const uint32_t *__restrict__ lo_of,
                                                      unsigned long long n_pairs, int32_t thr, uint2 *__restrict__ surv, unsigned long long surv_cap,
                                                      unsigned long long *__restrict__ ctr)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool live = p < n_pairs;
    uint32_t a = 0, b = 0;
    int32_t m = 0, nb = 0, d_first = thr + 1;
    EinvHead ha = {0ull, 0ull}, hb = {0ull, 0ull};
    if (live) {
        a = einv_owner(first, S.n, p);
        b = einv_slot_partner(a, lo_of[a], (uint32_t)(p - first[a]));
        m = S.lens[a];
        nb = S.lens[b];
        d_first = einv_first_shift(m, nb, thr);
        ha = einv_head(S.planes, S.n, S.nchunks, a);
        hb = einv_head(S.planes, S.n, S.nchunks, b);
    }
    const int32_t d_wave = wave_min_i32(d_first);
    bool any = false;
    for (int32_t d = d_wave; d <= thr; ++d) {
        const bool ok = live && d >= d_first && einv_first_word_matches(S.planes, S.n, S.nchunks, a, m, b, nb, d, ha, hb);
        const unsigned long long mask = __ballot(ok);
        if (!mask) continue;          // (wave-uniform)
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(ctr + EINV_SURVIVORS, (unsigned long long)__popcll(mask));
        base = __shfl(base, 0, 64);
        if (ok) {
            const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < surv_cap) surv[at] = make_uint2((uint32_t)p, (uint32_t)d);
            any = true;
        }
    }
    const unsigned long long with = __ballot(any);
    if (lane == 0 && with) atomicAdd(ctr + EINV_VERIFIED, (unsigned long long)__popcll(with));
}

__global__ __launch_bounds__(256) void k_einv_verify(DevStore S, const unsigned long long *__restrict__ first, const uint32_t *__restrict__ lo_of,
                                                      const uint2 *__restrict__ surv, unsigned long long n_surv, uint32_t *__restrict__ best)
{
    const unsigned long long x = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (x >= n_surv) return;
    const uint2 rec = surv[x];
    const uint32_t a = einv_owner(first, S.n, rec.x), b = einv_slot_partner(a, lo_of[a], (uint32_t)(rec.x - first[a]));
    const int32_t m = S.lens[a], nb = S.lens[b], d = (int32_t)rec.y;
    if (einv_match(S.planes, S.n, S.nchunks, a, m, b, nb, d)) atomicMin(best + rec.x, einv_key(m, nb, d));
}

// WRITE false: row_count[i] = entries of row i.  WRITE true: the entries, from row_ptr[i] on.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_einv_rows(const int32_t *__restrict__ lens, const unsigned long long *__restrict__ first, const uint32_t *__restrict__ lo_of,
                                                    uint32_t n, int32_t thr, const uint32_t *__restrict__ best, uint32_t *__restrict__ row_count,
                                                    const unsigned long long *__restrict__ row_ptr, uint32_t *__restrict__ cols)
{
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    const unsigned long long base = first[i], below = (1ull << lane) - 1ull;
    const uint32_t tot = (uint32_t)(first[i + 1] - base), lo = lo_of[i];
    const int32_t m = lens[i];
    const unsigned long long w0 = WRITE ? row_ptr[i] : 0ull;
    uint32_t count = 0;
    for (uint32_t r0 = 0; r0 < tot; r0 += 64u) {
        const uint32_t r = r0 + lane;
        uint32_t b = 0;
        bool inv = false;
        if (r < tot) {
            b = einv_slot_partner(i, lo, r);
            inv = einv_invariant(m, lens[b], thr, best[base + r]);
        }
        const unsigned long long mask = __ballot(inv);
        if (WRITE && inv) cols[w0 + count + (uint32_t)__popcll(mask & below)] = b;
        count += (uint32_t)__popcll(mask);
    }
    if (!WRITE && lane == 0) row_count[i] = count;
}

}  // namespace isocon
