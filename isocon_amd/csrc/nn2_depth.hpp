// nn2_depth.hpp -- kernels of the depth-limited reads x candidates search (nn2_depth_core.hpp holds the lane routines and the scheme;
// the host driver is nn2_depth.inc).  One lane per read; the state of the reads is a structure of arrays indexed by the read's rank r
// among the reads.  Replaces the loop /root/reference/modules/nearest_neighbor_graph.py:341-424 for neighbor_search_depth smaller than
// the number of candidates.
#pragma once
#include "common.hpp"
#include "nn2_depth_core.hpp"

namespace isocon {

struct NN2State {
    const uint32_t *qidx, *tiq;          // the read's entry, the number of targets below it
    uint32_t *a, *b;
    int32_t *best;
    uint32_t *processed, *flags;
    uint32_t *jend, *pbase, *pcnt;       // this round: last event listed, the read's slots in the pair arrays
    uint32_t nq;
    __device__ __forceinline__ NN2Lane load(uint32_t r) const { return NN2Lane{a[r], b[r], best[r], processed[r], flags[r]}; }
    __device__ __forceinline__ void store(uint32_t r, const NN2Lane &L) const { a[r] = L.a; b[r] = L.b; best[r] = L.best; processed[r] = L.processed; flags[r] = L.flags; }
};

// the pairs of a round: read, target, frozen best, the threshold of the 64-row kernel (-1: not for it), distance
struct NN2Pairs {
    uint32_t *pa, *pb;
    int32_t *pk, *pk_lanes, *pd;
    unsigned long long cap;
};

// counters of a round (device, 8 bytes each)
enum { NN2_CTR_PAIRS = 0, NN2_CTR_OPEN, NN2_CTR_WIDE, NN2_CTR_BYTES, NN2_CTR_ERROR, NN2_CTR_COUNT };

// Step 1.  A lane walks its events twice: once to count (the slots of a read are contiguous, reserved with one atomic), once to write.
// exc: entries the bit-vector kernels must not see (nullptr: none).
__global__ __launch_bounds__(256) void k_nn2_speculate(NN2Set S, NN2State T, uint32_t B, NN2Pairs Q, const uint8_t *__restrict__ exc,
                                                        unsigned long long *__restrict__ ctr)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= T.nq) return;
    const NN2Lane L = T.load(r);
    const uint32_t i = T.qidx[r], ti = T.tiq[r];
    uint32_t j_end = 0;
    const uint32_t cnt = nn2_speculate(S, i, ti, L, B, j_end, [](uint32_t) {});
    unsigned long long at = cnt ? atomicAdd(ctr + NN2_CTR_PAIRS, (unsigned long long)cnt) : 0ull;
    T.jend[r] = j_end;
    if (at + cnt > Q.cap) {          // (the host sizes the arrays for B + 1 pairs per open read: cannot happen)
        atomicAdd(ctr + NN2_CTR_ERROR, 1ull);
        T.pbase[r] = 0;
        T.pcnt[r] = 0;
        return;
    }
    T.pbase[r] = (uint32_t)at;
    T.pcnt[r] = cnt;
    if (!cnt) return;
    const bool exc_i = exc != nullptr && exc[i] != 0;
    nn2_speculate(S, i, ti, L, B, j_end, [&](uint32_t p) {
        Q.pa[at] = i;
        Q.pb[at] = p;
        Q.pk[at] = L.best;
        Q.pk_lanes[at] = (exc_i || (exc != nullptr && exc[p] != 0)) ? -1 : L.best;
        Q.pd[at] = -1;
        ++at;
    });
}

// Step 2, after k_ed_lanes<false> over the round's pairs: the pairs the 64-row band could not decide (threshold above 63 and no
// distance <= 63, or an entry outside the planes' map) are compacted for the widening stages of ed_pairs_impl.
__global__ __launch_bounds__(256) void k_nn2_undecided(NN2Pairs Q, unsigned long long n_pairs, uint32_t *__restrict__ oa, uint32_t *__restrict__ ob,
                                                        int32_t *__restrict__ ok, uint32_t *__restrict__ oidx, unsigned long long *__restrict__ ctr)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    if (Q.pd[p] >= 0 || (Q.pk_lanes[p] >= 0 && Q.pk[p] <= 63)) return;
    if (Q.pk_lanes[p] < 0) atomicAdd(ctr + NN2_CTR_BYTES, 1ull);          // (an entry outside the planes' map: k_ed_bytes)
    const unsigned long long at = atomicAdd(ctr + NN2_CTR_WIDE, 1ull);          // (at < n_pairs: the arrays have the size of the pair arrays)
    oa[at] = Q.pa[p];
    ob[at] = Q.pb[p];
    ok[at] = Q.pk[p];
    oidx[at] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void k_nn2_scatter(const uint32_t *__restrict__ oidx, const int32_t *__restrict__ ores, unsigned long long n_wide,
                                                      unsigned long long n_pairs, int32_t *__restrict__ pd)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (t >= n_wide) return;
    const uint32_t p = oidx[t];
    if (p < n_pairs) pd[p] = ores[t];
}

// Step 3.  Hits (read, target, d) join the search's hit list: the CSR routines keep the ones that attain the read's final best[] and
// order them the way the reference inserts (ascending offset, the lower index first -- the order of the visits).
__global__ __launch_bounds__(256) void k_nn2_replay(NN2Set S, NN2State T, NN2Pairs Q, int32_t *__restrict__ best_of_entry, int32_t *__restrict__ hits,
                                                     unsigned long long *__restrict__ hit_count, unsigned long long hits_cap,
                                                     unsigned long long *__restrict__ ctr)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= T.nq) return;
    NN2Lane L = T.load(r);
    if (L.flags & NN2_DONE) return;
    const uint32_t i = T.qidx[r], base = T.pbase[r];
    nn2_replay(S, i, T.tiq[r], L, T.jend[r], Q.pb + base, Q.pd + base, T.pcnt[r], [&](uint32_t p, int32_t d) {
        const unsigned long long at = atomicAdd(hit_count, 1ull);
        if (at < hits_cap) {
            hits[at * 3] = (int32_t)i;
            hits[at * 3 + 1] = (int32_t)p;
            hits[at * 3 + 2] = d;
        }
    });
    T.store(r, L);
    best_of_entry[i] = L.best;
    if (L.flags & NN2_ERROR) atomicAdd(ctr + NN2_CTR_ERROR, 1ull);
    if (!(L.flags & NN2_DONE)) atomicAdd(ctr + NN2_CTR_OPEN, 1ull);
}

}  // namespace isocon
