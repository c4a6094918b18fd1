// nn_surv_core.hpp -- where the kept pairs of one batch of the survivor-list builder (nn_list.hpp, k_nn_survivors) go in the staging
// buffer, and when a chunk leaves it.  Shared by the kernel and its CPU emulator (tests/emul/survivor_groups_emul.cpp).
//
// A batch is 256 consecutive row positions: lane l holds the positions 4 l + b, b = 0 .. 3, so the 16 lanes 16 j .. 16 j + 15 hold
// the 64 consecutive positions of GROUP j.  The builder used to take 64 positions per step and to ask after every step whether the
// buffer had reached a chunk; the chunks (their owner, their pair sets, their class) decide what the block filter does with them, so
// the batch asks the same question at the same places: after every group, in the order of the groups.
// The keep masks come as one ballot per b and class: bit l of m[b] = the pair at position 4 l + b is kept in that class.
#pragma once
#include "band_core.hpp"

namespace isocon {

static constexpr int SURV_PER_LANE = 4;                 // row positions per lane and batch
static constexpr int SURV_GROUPS = 4;                   // groups of 16 lanes = 64 positions
static constexpr int SURV_BATCH = 64 * SURV_PER_LANE;

// the lanes of group j
ISO_HD uint64_t surv_group_lanes(int j) { return (uint64_t)0xffffu << (16 * j); }

// kept pairs of one class at the given lanes
ISO_HD uint32_t surv_count(const uint64_t (&m)[SURV_PER_LANE], uint64_t lanes)
{
    uint32_t c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int b = 0; b < SURV_PER_LANE; ++b) c += (uint32_t)popc64(m[b] & lanes);
    return c;
}

// kept pairs of one class at the lanes below `lane` (device: the executing lane; v_mbcnt counts the mask bits below it)
ISO_HD uint32_t surv_rank(const uint64_t (&m)[SURV_PER_LANE], int lane)
{
    uint32_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
#pragma unroll
    for (int b = 0; b < SURV_PER_LANE; ++b) r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m[b] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[b], r));
#else
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int b = 0; b < SURV_PER_LANE; ++b) r += (uint32_t)popc64(m[b] & below);
#endif
    return r;
}

// bit `lane` of a lane mask as 0 / 1 (device: the executing lane, one select on the mask)
ISO_HD uint32_t surv_lane_bit(uint64_t m, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(m));
    return r;
#else
    return (uint32_t)(m >> lane) & 1u;
#endif
}

// Where a lane's kept pairs of one class go: the pairs of a write are numbered in the order of their positions, (l, b) ascending, from
// `off` (as handed to the write callback of surv_batch) -- the first of lane l at off + surv_rank(m, l), its next ones behind it.

// One batch.  am, an: keep masks of the 64-row and of the 32-row class; fill, fill_n: pairs of each class in the buffer.
//   write(lanes, off_a, off_n)   the lanes in `lanes` store their kept pairs: 64-row class from index off_a + surv_rank(am, l) of the front,
//                                32-row class from index off_n + surv_rank(an, l) of the back
//   flush(narrow)                the buffer holds `chunk` pairs or more: its larger class leaves (the callback empties it: fill or fill_n = 0)
// A batch that does not fill the buffer is one write of all lanes; otherwise the groups are written one after the other with the
// check behind each of them -- the flush points of 64 positions per step.
template <class Write, class Flush>
ISO_HD void surv_batch(const uint64_t (&am)[SURV_PER_LANE], const uint64_t (&an)[SURV_PER_LANE], uint32_t &fill, uint32_t &fill_n, uint32_t chunk, Write write, Flush flush)
{
    const uint32_t ca = surv_count(am, ~(uint64_t)0), cn = surv_count(an, ~(uint64_t)0);
    if (ca + cn == 0) return;
    if (fill + fill_n + ca + cn < chunk) {
        write(~(uint64_t)0, fill, fill_n);
        fill += ca;
        fill_n += cn;
        return;
    }
    uint32_t before_a = 0, before_n = 0;          // kept pairs of the groups in front of j
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1          // (one copy of the callbacks: a batch that fills the buffer is one in hundreds)
#endif
    for (int j = 0; j < SURV_GROUPS; ++j) {
        const uint64_t lanes = surv_group_lanes(j);
        const uint32_t ga = surv_count(am, lanes), gn = surv_count(an, lanes);
        if (ga + gn != 0) {
            write(lanes, fill - before_a, fill_n - before_n);          // (modulo 2^32: the lanes add their rank, which is >= before)
            fill += ga;
            fill_n += gn;
            if (fill + fill_n >= chunk) flush(fill_n > fill);
        }
        before_a += ga;
        before_n += gn;
    }
}

}  // namespace isocon
