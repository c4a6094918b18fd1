// hw_graph.hpp -- the candidate-vs-candidate graph with ignored ends built on the device (isocon_hw_window_graph): device side of
// get_all_NN (modules/end_invariant_functions.py:622-681 of the reference), the end rules of edlib_traceback (:593-620) and the
// symmetrisation of get_NN_graph_ignored_ends_edlib (:757-788).  Index arithmetic: hw_graph_core.hpp.
//   k_hwg_counts   one thread per entry: its neighbours below / above (two binary searches in the sorted lengths, the depth cap)
//   k_hwg_pairs    one thread per slot: query, target and threshold of the pair (closed form of the entry's counts and the slot)
//   -- the rows of all pairs: the tile builder and the LOCATE / START / TRACE kernels of isocon_hw_pairs (hw_tiles.hpp, hw.hpp) --
//   k_hwg_adjust   one thread per pair: the end rules on its row -> the value of the directed edge, or -1
//   k_hwg_edges    one wavefront per entry, a count pass and a write pass: the entry's directed edges in visit order (ballot
//                  compaction), for the symmetric form with the smaller of the two directions' values, then the neighbours that only
//                  have an edge TO the entry, in ascending position
// No LDS, no atomics on the result: a row is written by one wavefront in its final order.
#pragma once
#include "common.hpp"
#include "hw_graph_core.hpp"

namespace isocon {

// counters of one call, zeroed by the host
enum { HWG_PAIRS = 0, HWG_NEED_KERNEL, HWG_HITS, HWG_DIRECTED, HWG_APPENDED, HWG_COUNTERS };

__global__ __launch_bounds__(256) void k_hwg_counts(const int32_t *__restrict__ lens, uint32_t n, int32_t window, uint32_t jmax, uint32_t *__restrict__ cd_out,
                                                     uint32_t *__restrict__ tot_out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t cd, cu;
    hwg_counts(lens, n, i, window, jmax, cd, cu);
    cd_out[i] = cd;
    tot_out[i] = cd + cu;
}

// first[i] = slots before entry i (first[n] = n_pairs)
__global__ __launch_bounds__(256) void k_hwg_pairs(const unsigned long long *__restrict__ first, const uint32_t *__restrict__ cd_of, uint32_t n,
                                                    unsigned long long n_pairs, int32_t k, uint32_t *__restrict__ q, uint32_t *__restrict__ t, int32_t *__restrict__ pk)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    // the last entry whose first slot is <= p (entries without a slot share their successor's first slot)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t i = lo, cd = cd_of[i], cu = (uint32_t)(first[i + 1] - first[i]) - cd;
    q[p] = i;
    t[p] = hwg_slot_target(i, cd, cu, (uint32_t)(p - first[i]));
    pk[p] = k;
}

template <class T>
__device__ __forceinline__ T hwg_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_hwg_adjust(const int32_t *__restrict__ lens, const uint32_t *__restrict__ q, const uint32_t *__restrict__ t,
                                                     const int32_t *__restrict__ rows, unsigned long long n_pairs, int32_t k, int32_t end_threshold, int32_t max_ed,
                                                     int32_t *__restrict__ value, unsigned long long *__restrict__ ctr)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    uint32_t need = 0, hit = 0, edge = 0;
    if (p < n_pairs) {
        const int32_t lq = lens[q[p]], lt = lens[t[p]];
        int32_t row[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) row[c] = rows[p * 5 + c];
        const int32_t v = hwg_edge_value(row, lt, end_threshold, max_ed);
        value[p] = v;
        need = !(lt - lq < -k || lq == 0 || lt == 0);          // (k_hwt_keys<0>: the pairs that get a tile)
        hit = row[0] >= 0;
        edge = v >= 0;
    }
    const uint32_t packed = hwg_wave_sum(need | (hit << 8) | (edge << 16));          // (64 lanes: each field stays below 256)
    if ((threadIdx.x & 63u) == 0 && packed) {
        if (packed & 0xffu) atomicAdd(ctr + HWG_NEED_KERNEL, (unsigned long long)(packed & 0xffu));
        if ((packed >> 8) & 0xffu) atomicAdd(ctr + HWG_HITS, (unsigned long long)((packed >> 8) & 0xffu));
        if ((packed >> 16) & 0xffu) atomicAdd(ctr + HWG_DIRECTED, (unsigned long long)((packed >> 16) & 0xffu));
    }
}

// the value of the edge t -> i (-1: none): the slot of i in the list of t
__device__ __forceinline__ int32_t hwg_reverse_value(const unsigned long long *__restrict__ first, const uint32_t *__restrict__ cd_of, const int32_t *__restrict__ value,
                                                     uint32_t i, uint32_t t)
{
    const unsigned long long ft = first[t];
    const uint32_t cdt = cd_of[t], cut = (uint32_t)(first[t + 1] - ft) - cdt;
    return value[ft + hwg_slot_of(t, cdt, cut, i)];
}

// WRITE false: row_count[i] = entries of row i.  WRITE true: the entries, from row_ptr[i] on.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hwg_edges(const unsigned long long *__restrict__ first, const uint32_t *__restrict__ cd_of, uint32_t n,
                                                    const int32_t *__restrict__ value, int32_t symmetric, uint32_t *__restrict__ row_count,
                                                    const unsigned long long *__restrict__ row_ptr, uint32_t *__restrict__ cols, int32_t *__restrict__ ed,
                                                    unsigned long long *__restrict__ ctr)
{
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    const unsigned long long base = first[i], below = (1ull << lane) - 1ull;
    const uint32_t cd = cd_of[i], tot = (uint32_t)(first[i + 1] - base), cu = tot - cd;
    const unsigned long long w0 = WRITE ? row_ptr[i] : 0ull;
    uint32_t count = 0, appended = 0;
    // the directed edges i -> t in visit order
    for (uint32_t r0 = 0; r0 < tot; r0 += 64u) {
        const uint32_t r = r0 + lane;
        uint32_t t = 0;
        int32_t v = -1;
        if (r < tot) {
            t = hwg_slot_target(i, cd, cu, r);
            v = value[base + r];
            if (symmetric && v >= 0) {
                const int32_t back = hwg_reverse_value(first, cd_of, value, i, t);
                if (back >= 0 && back < v) v = back;
            }
        }
        const unsigned long long m = __ballot(v >= 0);
        if (WRITE && v >= 0) {
            const unsigned long long at = w0 + count + (uint32_t)__popcll(m & below);
            cols[at] = t;
            ed[at] = v;
        }
        count += (uint32_t)__popcll(m);
    }
    // the neighbours with an edge t -> i and none i -> t, in ascending position
    if (symmetric) {
        for (uint32_t x0 = 0; x0 < tot; x0 += 64u) {
            const uint32_t x = x0 + lane;
            uint32_t t = 0;
            int32_t v = -1;
            if (x < tot) {
                t = i - cd + x + (x >= cd ? 1u : 0u);
                if (value[base + hwg_slot_of(i, cd, cu, t)] < 0) v = hwg_reverse_value(first, cd_of, value, i, t);
            }
            const unsigned long long m = __ballot(v >= 0);
            if (WRITE && v >= 0) {
                const unsigned long long at = w0 + count + (uint32_t)__popcll(m & below);
                cols[at] = t;
                ed[at] = v;
            }
            count += (uint32_t)__popcll(m);
            appended += (uint32_t)__popcll(m);
        }
    }
    if (!WRITE && lane == 0) {
        row_count[i] = count;
        if (appended) atomicAdd(ctr + HWG_APPENDED, (unsigned long long)appended);
    }
}

}  // namespace isocon
