// nn2_depth.hpp -- kernels of the depth-limited reads x candidates search (nn2_depth_core.hpp holds the lane routines and the scheme;
// the host driver is nn2_depth.inc).  One lane per read; the state of the reads is a structure of arrays indexed by the read's rank r
// among the reads.  Replaces the loop /root/reference/modules/nearest_neighbor_graph.py:341-424 for neighbor_search_depth smaller than
// the number of candidates.
#pragma once
#include "common.hpp"
#include "nn2_depth_core.hpp"
#include "nn_filter.hpp"

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

// counters of a round (device, 8 bytes each); TASKS .. SURVIVORS belong to the block test: tasks made, the queue's cursor, pairs
// rejected, pairs left for the pair-per-lane launch
enum { NN2_CTR_PAIRS = 0, NN2_CTR_OPEN, NN2_CTR_WIDE, NN2_CTR_BYTES, NN2_CTR_ERROR, NN2_CTR_TASKS, NN2_CTR_TASK_NEXT, NN2_CTR_REJECTED, NN2_CTR_SURVIVORS,
       NN2_CTR_COUNT };
static_assert(NN2_B_MAX + 1 <= NN2_TASK_PAIRS, "a read's pairs of one round are one task: the driver sizes the task array with one per open read");

// Step 1.  A lane walks its events twice: once to count (the slots of a read are contiguous, reserved with one atomic), once to write.
// exc: entries the bit-vector kernels must not see (nullptr: none).  tasks (nullptr: the round runs without the block test): the lane
// cuts its run into tasks for k_nn2_block_reject -- none if the test can reject none of its pairs (nn2_tested), as in the first round.
__global__ __launch_bounds__(256) void k_nn2_speculate(NN2Set S, NN2State T, uint32_t B, NN2Pairs Q, const uint8_t *__restrict__ exc,
                                                        unsigned long long *__restrict__ ctr, NN2Task *__restrict__ tasks, unsigned long long tasks_cap)
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
    if (tasks == nullptr) return;
    nn2_cut_tasks(T.pbase[r], cnt, [&](unsigned long long p) { return nn2_tested(Q.pk_lanes[p], S.lens[Q.pb[p]]); },
                  [&](unsigned long long first, uint32_t pairs) {
                      const unsigned long long ti = atomicAdd(ctr + NN2_CTR_TASKS, 1ull);
                      if (ti < tasks_cap) tasks[ti] = NN2Task{i, pairs, first};
                      else atomicAdd(ctr + NN2_CTR_ERROR, 1ull);
                  });
}

// Step 1b, the block test (nn_filter.hpp; modelled on k_nn_block_filter2).  A wave takes a task from the queue (a counter; waves never wait
// for each other), files the read's 8-grams in its own 8 KB bitmap and gives every pair of the task a lane: the greedy count of the
// target's grams that occur nowhere in the read, probes S bases apart, against k = the pair's frozen best.  count > k: the distance
// exceeds k, the pair is final with the -1 its slot holds and is marked NN2_REJECTED -- neither the pair-per-lane launch (k_nn2_survivors)
// nor k_nn2_undecided sees it.  Lanes whose pair is not tested (nn2_tested) idle.  tasks[ti], ti < n_tasks: ranges inside the pair arrays.
template <int S>
__global__ __launch_bounds__(256, 3) void k_nn2_block_reject(const uint32_t *__restrict__ text, uint32_t stride, const int32_t *__restrict__ lens,
                                                             const NN2Task *__restrict__ tasks, unsigned long long n_tasks, const uint32_t *__restrict__ pb,
                                                             int32_t *__restrict__ pk_lanes, unsigned long long *__restrict__ ctr)
{
    __shared__ uint32_t bitmaps[4][2048];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *bitmap = bitmaps[wave];
    for (;;) {
        unsigned long long ti = 0;
        if (lane == 0) ti = atomicAdd(ctr + NN2_CTR_TASK_NEXT, 1ull);
        ti = nnf_uniform64(ti);
        if (ti >= n_tasks) break;
        const NN2Task t = tasks[ti];
        const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.read);
        uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.count);
        count = count < NN2_TASK_PAIRS ? count : NN2_TASK_PAIRS;
        const unsigned long long begin = nnf_uniform64(t.begin);
        for (int i = lane; i < 2048; i += 64) bitmap[i] = 0xffffffffu;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        nnf_add_grams(bitmap, text + (size_t)x * stride, lens[x], lane, 64);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const bool listed = (uint32_t)lane < count;
        const unsigned long long p = begin + (unsigned long long)lane;
        const uint32_t y = listed ? pb[p] : 0u;
        const int32_t k = listed ? pk_lanes[p] : -1;
        const int32_t ly = lens[y];
        const bool active = listed && nn2_tested(k, ly);
        const uint32_t cnt = nnf_count<S>(bitmap, text + (size_t)y * stride, active ? nnf_dwords<S>(ly) : 0, k, active);
        const bool reject = active && (int32_t)cnt > k;
        if (reject) pk_lanes[p] = NN2_REJECTED;
        const uint32_t nr = (uint32_t)__popcll(__ballot(reject));
        if (lane == 0 && nr) atomicAdd(ctr + NN2_CTR_REJECTED, (unsigned long long)nr);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // (the next task's bitmap writes behind this task's reads)
    }
}

// workgroups of the test's launch (four waves each, a task per wave at a time)
inline unsigned nn2_reject_grid(unsigned long long n_tasks) { return (unsigned)std::min<unsigned long long>((n_tasks + 3) / 4, NNF_GRID2); }

template <int S>
inline hipError_t nn2_launch_reject(const uint32_t *text, uint32_t stride, const int32_t *lens, const NN2Task *tasks, unsigned long long n_tasks, const uint32_t *pb,
                                    int32_t *pk_lanes, unsigned long long *ctr)
{
    hipLaunchKernelGGL(k_nn2_block_reject<S>, dim3(nn2_reject_grid(n_tasks)), dim3(256), 0, 0, text, stride, lens, tasks, n_tasks, pb, pk_lanes, ctr);
    return hipGetLastError();
}

// ... and the pairs it left, dense, for k_ed_lanes<false> (a lane whose pair is merely masked would idle beside 63 working ones): a
// ballot and one atomic per wave; sidx = the pair's slot, for k_nn2_scatter.  Their number stays on the device (ctr[NN2_CTR_SURVIVORS]).
__global__ __launch_bounds__(256) void k_nn2_survivors(NN2Pairs Q, unsigned long long n_pairs, uint32_t *__restrict__ sa, uint32_t *__restrict__ sb,
                                                        int32_t *__restrict__ sk, uint32_t *__restrict__ sidx, unsigned long long *__restrict__ ctr)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool keep = p < n_pairs && Q.pk_lanes[p] != NN2_REJECTED;
    const uint64_t km = __ballot(keep);
    if (km == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr + NN2_CTR_SURVIVORS, (unsigned long long)__popcll(km));
    base = nnf_uniform64(base);
    if (!keep) return;
    const unsigned long long at = base + (unsigned long long)__popcll(km & (((uint64_t)1 << lane) - 1));          // (at < n_pairs)
    sa[at] = Q.pa[p];
    sb[at] = Q.pb[p];
    sk[at] = Q.pk_lanes[p];
    sidx[at] = (uint32_t)p;
}

// Step 2, after k_ed_lanes<false> over the round's pairs: the pairs the 64-row band could not decide (threshold above 63 and no
// distance <= 63, or an entry outside the planes' map) are compacted for the widening stages of ed_pairs_impl.  A pair the block test
// has rejected is decided.
__global__ __launch_bounds__(256) void k_nn2_undecided(NN2Pairs Q, unsigned long long n_pairs, uint32_t *__restrict__ oa, uint32_t *__restrict__ ob,
                                                        int32_t *__restrict__ ok, uint32_t *__restrict__ oidx, unsigned long long *__restrict__ ctr)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    if (Q.pd[p] >= 0 || (Q.pk_lanes[p] >= 0 && Q.pk[p] <= 63) || Q.pk_lanes[p] == NN2_REJECTED) return;
    if (Q.pk_lanes[p] < 0) atomicAdd(ctr + NN2_CTR_BYTES, 1ull);          // (an entry outside the planes' map: k_ed_bytes)
    const unsigned long long at = atomicAdd(ctr + NN2_CTR_WIDE, 1ull);          // (at < n_pairs: the arrays have the size of the pair arrays)
    oa[at] = Q.pa[p];
    ob[at] = Q.pb[p];
    ok[at] = Q.pk[p];
    oidx[at] = (uint32_t)p;
}

// live (nullptr: none): the number of entries as the device knows it, where the host only has an upper bound (n_wide)
__global__ __launch_bounds__(256) void k_nn2_scatter(const uint32_t *__restrict__ oidx, const int32_t *__restrict__ ores, unsigned long long n_wide,
                                                      unsigned long long n_pairs, int32_t *__restrict__ pd, const unsigned long long *__restrict__ live = nullptr)
{
    if (live != nullptr) { const unsigned long long nl = *live; n_wide = nl < n_wide ? nl : n_wide; }
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
