// nn_list.hpp -- the main pass of the nearest-neighbour search as LISTS: which pairs survive their q-gram bound is decided in one
// streaming pass over the bound matrix, the alignment kernels only see survivors, and every survivor is aligned against the
// match-mask table of whichever of its two ends has more pairs.
//
// Why (C3, 50 000 reads, measured: profiles/r03b_survivor_graph.txt): of the 3.5 10^8 window pairs ~1.1 10^7 survive (bound <= threshold),
// and they are spread very unevenly -- per entry as the lower index: median 22, 75 % 123, 90 % 449, 99 % 3 716, largest 10 904 (reads with
// few errors are near everybody).  A workgroup per entry that walks its whole window inside the alignment kernel (~110 batches of
// dependent loads per entry) spends its life finding 22 pairs and then runs them on 256 lanes; a 48 KB table in LDS pays only
// when hundreds of lanes use it.  Distances are symmetric, so a pair may use either end's table: handing every pair to the end of
// larger degree puts 88 % of the pairs into lists of >= 512 (73 % by lower index).
// Grouping pairs by an end that is not the row they were found in is a sparse transposition (two scattered atomics per pair: measured
// 4.8 ms for 1.3 10^7 pairs); instead k_qgram_mm also writes the TRANSPOSED matrix and a hub score per entry (pairs with a small
// bound, counted in its epilogue), so that ONE pass finds every entry's pairs on both sides and both ends of a pair agree on
// its owner without communicating:
//   1. k_nn_survivors   one wave per entry: its row and its transposed row through the in-kernel admission's tests (roles, window,
//                       threshold from the same best[], bound); the pairs it owns are staged in LDS and leave as chunks of a list
//                       (one k_nn_scan_refill workgroup per chunk: the entry's table in LDS, lanes refilled from the chunk) or, for
//                       entries with few pairs, as flat pairs for the one-pair-per-lane kernel (ed_lanes.hpp: no table);
//   2. the block filter on the chunks (nn_filter.hpp), then the alignment launches on what it leaves (nn_lists.inc, nn_main.inc).
// The pair set is exactly the one the in-kernel admission evaluates, so the graph is unchanged; replaces the window walk of
// /root/reference/modules/nearest_neighbor_graph.py:136-178.
#pragma once
#include "nn.hpp"
#include "nn_surv_core.hpp"

namespace isocon {

static constexpr uint32_t NN_LIST_MIN = 256;       // owners with fewer pairs (and what is left of a list below this): one pair per lane
#ifndef ISOCON_NN_LIST_CHUNK          // (experiments build the library with another value: scripts/dev/build_variant.sh)
#define ISOCON_NN_LIST_CHUNK 2048
#endif
static constexpr uint32_t NN_LIST_CHUNK = ISOCON_NN_LIST_CHUNK;    // a wave hands over a chunk as soon as it has staged this many pairs of its entry
static constexpr int NN_STAGE = NN_LIST_CHUNK + 64;
#ifndef ISOCON_SURV_WAVES            // waves (= entries) per workgroup of the list builder.  One: 8.4 KB of LDS per workgroup, so residency is bound by
#define ISOCON_SURV_WAVES 1          // registers (24 waves per CU) instead of LDS (16 with four): 1.06 -> 0.98 ms at C3 (profiles/r05t_chunk_sweep.txt)
#endif
static constexpr int NN_SURV_WAVES = ISOCON_SURV_WAVES;

// counters of the list builder, each on a cache line of its own (they are hot: tens of thousands of atomics per launch)
struct NNPlanTotals {
    unsigned long long n_pairs, pad0[15], n_list, pad1[15], n_small, pad2[15], n_chunks, pad3[15], n_filtered, pad4[15], overflow, pad5[15];
    unsigned long long n_chunks_narrow, pad6[15];          // chunks of the 32-row class (n_chunks counts the 64-row class)
    unsigned long long n_wide_pairs, n_narrow_listed, pad7[14];          // pairs sent to the pair-per-lane kernel for their threshold (class mode 1); pairs in narrow chunks
    // the block filter behind the list builder (nn_filter.hpp): its work queue, the chunks it leaves per class, the pairs it rejected
    unsigned long long f_next, pad8[15], f_chunks, pad9[15], f_chunks_narrow, pad10[15], f_rejected, f_narrow_listed, f_listed, f_rejected2, pad11[12];          // f_listed: pairs in the chunks it leaves (both classes); f_rejected2: by its second pass
    unsigned long long f_tasks, pad12[15], f_task_next, pad13[15];          // tasks of the second pass (nn_filter.hpp) and its queue
    unsigned long long n_seed_known, pad14[15];          // flat pairs that the seed pass of the call had aligned already (NNSeedKnown)
};

// The seed pairs of the call as a table (written by k_qgram_seed_pairs, qgram_mm.hpp): known[x][0 .. NN_KNOWN_SLOTS) = the other ends of the
// pairs thread x proposed, 0xffffffff = none.  A pair (a, b) is SETTLED iff b is in known[a] or a is in known[b] (the column candidate a
// thread drops because the row proposes the same pair is in the row's entry).  The seed pass aligned a settled pair under a threshold
// that was at least the one the main pass would use (best[] only decreases, same roles, same min_d) and is through before the lists are
// built: a hit is in the hit list already, a miss stays a miss.  So the kernels that make FLAT pairs -- after every decision of the
// filters, which see and count a settled pair as ever -- leave it out of the pair arrays (drop != 0) or only count it (drop == 0:
// nn_seed_skip=0 / =count).  known == nullptr: no table (2-set, is_converged, fixed thresholds, images, seeds of another call).
static constexpr uint32_t NN_KNOWN_SLOTS = 8;
struct NNSeedKnown { const uint32_t *known; uint32_t drop; };
typedef uint32_t NNKnownRow __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool nn_seed_known(const uint32_t *__restrict__ known, uint32_t a, uint32_t b)
{
    const NNKnownRow *ra = reinterpret_cast<const NNKnownRow *>(known + (size_t)a * NN_KNOWN_SLOTS), *rb = reinterpret_cast<const NNKnownRow *>(known + (size_t)b * NN_KNOWN_SLOTS);
    const NNKnownRow a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
    bool hit = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) hit = hit || a0[i] == b || a1[i] == b || b0[i] == a || b1[i] == a;
    return hit;
}

// Threshold classes of the listed launch.  A pair whose threshold max(k of its two directions) is <= NN_NARROW_K is exact on 32
// diagonals (a path of cost <= k stays inside k + 1 of them), and on 32-bit vectors the table kernel's column is 12 instead of 21
// instructions with one table dword instead of two (nn.hpp, HALF).  The class is decided PER PAIR: the list builder files the pairs of
// an entry under their class, a chunk holds one class, and the host launches k_nn_scan_refill<.., true> over the narrow chunks and
// <.., false> over the others.  (Round 3 decided per LAUNCH -- narrow only when fewer than n / 16 queries had a threshold above 31 --
// so C3, whose median threshold is 32, ran every pair on 64 rows.)
// class_mode: 0 = per pair; -1 = every pair in the 64-row class (A/B runs, tests); +1 = the pairs above NN_NARROW_K leave the lists
// for the one-pair-per-lane kernel, which takes any threshold up to 63 (the round-3 narrow mode, forced).
static constexpr int32_t NN_NARROW_K = 31;

// the matrix rows of both orientations (qgram_mm.hpp) and the hub scores that decide which end owns a pair
struct NNBoundRows {
    const uint8_t *lb;  const unsigned long long *row_off; const uint32_t *row_len;                      // row of slot s: columns p = q(s) + 1 ...
    const uint8_t *lbT; const unsigned long long *offT;    const uint32_t *sloT; const uint32_t *lenT;   // row of entry p: slots sloT[p] ...
    const uint32_t *score;
};

// what the scan needs to know about a partner, in ONE dword (the scan reads one per window pair and side: 7 10^8 at C3, L2 traffic):
// length (14 bits: the table kernel's limit is below), threshold min(best, length, 64) (7 bits: anything above 63 acts as 63),
// roles (2 bits: target, query), hub score >> 5 capped at 511 (9 bits: only orders the two ends of a pair, the same on both sides)
__device__ __forceinline__ uint32_t nn_meta_len(uint32_t w) { return w & 0x3fffu; }
__device__ __forceinline__ int32_t nn_meta_thr(uint32_t w) { return (int32_t)((w >> 14) & 0x7fu); }
__device__ __forceinline__ uint32_t nn_meta_score(uint32_t w) { return w >> 23; }
static constexpr uint32_t NN_META_PAD = 3;          // words behind the last entry's, all 0 (no roles: never a candidate): the scan loads four words at once
typedef uint32_t NNMeta4 __attribute__((ext_vector_type(4), aligned(4)));          // four meta words of consecutive entries: one 16-byte load at a dword address

// The same facts as the packed test of the scan wants them (nn_surv_core.hpp surv_test4: four partners per instruction), an item per entry
// in three arrays behind the meta words, each with the NN_META_PAD items of padding (no roles, guard bits set).  A lane loads the items
// of its four partners with one load per array, at any byte address.
struct NNSurvSide {
    const uint8_t *role, *len7;          // surv_role_byte (the cap of the pass folded in), surv_len_byte
    const uint16_t *score;               // surv_score_half
};
// the packed test needs every threshold + 1 in seven bits (and a length-sorted store: every caller's), and has no third class
static inline bool nn_surv_packed(int32_t kcap, int32_t class_mode) { return class_mode <= 0 && kcap >= 0 && kcap <= 63; }
static inline size_t nn_meta_bytes(size_t n) { return (n + NN_META_PAD) * 8; }          // meta words, score halves, role bytes, length bytes
static inline NNSurvSide nn_surv_side(uint32_t *meta, size_t n)
{
    NNSurvSide s;
    uint16_t *sc = reinterpret_cast<uint16_t *>(meta + (n + NN_META_PAD));
    uint8_t *role = reinterpret_cast<uint8_t *>(sc + (n + NN_META_PAD));
    s.score = sc; s.role = role; s.len7 = role + (n + NN_META_PAD);
    return s;
}

__global__ __launch_bounds__(256) void k_nn_entry_meta(DevStore S, NNParams P, const uint32_t *__restrict__ score, uint32_t *__restrict__ meta, NNSurvSide A, NNPlanTotals *__restrict__ totals)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= S.n && x < S.n + NN_META_PAD) {
        meta[x] = 0u;
        const_cast<uint8_t *>(A.role)[x] = 0;
        const_cast<uint8_t *>(A.len7)[x] = surv_len_byte(0);
        const_cast<uint16_t *>(A.score)[x] = surv_score_half(0);
    }
    if (x < S.n) {
        const int32_t m = S.lens[x], b = load_relaxed_agent(P.best + x);
        int32_t thr = b < m ? b : m;
        thr = thr < 64 ? thr : 64;
        const uint32_t sc = score[x] >> 5;
        const bool isq = P.qflag[x] != 0, ist = P.tflag[x] != 0;
        const uint32_t sc9 = sc < 511u ? sc : 511u;
        meta[x] = ((uint32_t)m & 0x3fffu) | ((uint32_t)thr << 14) | ((ist ? 1u : 0u) << 21) | ((isq ? 1u : 0u) << 22) | (sc9 << 23);
        const_cast<uint8_t *>(A.role)[x] = surv_role_byte(ist, isq, thr, P.kcap);
        const_cast<uint8_t *>(A.len7)[x] = surv_len_byte((uint32_t)m);
        const_cast<uint16_t *>(A.score)[x] = surv_score_half(sc9);
    }
}

// One wave per entry x.  Its pairs are the columns of its own row (partners above x; only if x is one of the launch slots) and the
// slots of its transposed row (partners below x): the same survival test from both sides (roles, length window, threshold from the
// same best[], bound), and the same ownership rule -- the end with the larger hub score, ties to the lower index -- so every
// surviving pair is kept by exactly one of its two ends.  Kept pairs are staged in LDS; NN_LIST_CHUNK staged pairs become a chunk
// of `list` (one k_nn_scan_refill workgroup with x's table), what is left at the end becomes a last chunk if it has NN_LIST_MIN
// pairs, else flat pairs for the one-pair-per-lane kernel -- those of them that the seed pass has not settled (K).
template <bool PACKED>
__global__ __launch_bounds__(64 * NN_SURV_WAVES) void k_nn_survivors(DevStore S, NNParams P, NNBoundRows B, const uint32_t *__restrict__ meta, NNSurvSide A, QMap Q, uint32_t nq,
                                                       uint32_t *__restrict__ list, unsigned long long list_cap, NNChunk *__restrict__ chunks, unsigned long long chunks_cap,
                                                       uint32_t *__restrict__ pa, uint32_t *__restrict__ pb, unsigned long long small_cap, NNPlanTotals *__restrict__ totals, uint32_t list_min,
                                                       int32_t class_mode, NNSeedKnown K)
{
    __shared__ uint32_t stage[NN_SURV_WAVES][NN_STAGE];
    __shared__ uint32_t s_small[NN_SURV_WAVES], s_filtered[NN_SURV_WAVES], s_kept[NN_SURV_WAVES], s_known[NN_SURV_WAVES];
    __shared__ unsigned long long s_base;
    const int wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * (uint32_t)NN_SURV_WAVES + (uint32_t)wave;
    const int lane = threadIdx.x & 63;
    const uint32_t mx = x < S.n ? meta[x] : 0u;
    const bool x_isq = (mx & (1u << 22)) != 0, x_ist = (mx & (1u << 21)) != 0;
    // x's own row, if it is a launch slot, and its transposed row
    uint32_t up_len = 0, dn_len = 0, dn_slo = 0;
    unsigned long long up_off = 0, dn_off = 0;
    if (x < S.n && (x_isq || x_ist)) {
        uint32_t s;
        if (Q.slot_of(x, s) && s < nq) {
            up_len = B.row_len[s];
            up_off = B.row_off[s];
        }
        dn_len = B.lenT[x]; dn_slo = B.sloT[x]; dn_off = B.offT[x];
    }
    if constexpr (PACKED && NN_SURV_WAVES == 1) {
        // (one entry per wave: what describes its rows is wave-uniform, and the loops over them are scalar when the compiler knows it)
        const auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
        up_len = uni(up_len); dn_len = uni(dn_len); dn_slo = uni(dn_slo);
        up_off = ((unsigned long long)uni((uint32_t)(up_off >> 32)) << 32) | uni((uint32_t)up_off);
        dn_off = ((unsigned long long)uni((uint32_t)(dn_off >> 32)) << 32) | uni((uint32_t)dn_off);
    }
    const int32_t m = (int32_t)nn_meta_len(mx);
    const int32_t kx0 = nn_meta_thr(mx);
    const uint32_t sx = nn_meta_score(mx);
    uint32_t *st = stage[wave];
    // the staging buffer holds both classes: the 64-row class grows from its front (fill), the 32-row class from its back (fill_n)
    uint32_t fill = 0, fill_n = 0, filtered = 0, kept = 0;
    // one class leaves as a chunk: the 64-row chunks in chunks[0 .. chunks_cap), the 32-row chunks in chunks[chunks_cap .. 2 chunks_cap)
    // (merged: what is left of the 32-row class leaves together with the 64-row class, as a 64-row chunk)
    auto emit_chunk = [&](bool narrow_class, bool merged = false) {
        const uint32_t cnt = merged ? fill + fill_n : narrow_class ? fill_n : fill;
        unsigned long long base = 0, ci = 0;
        if (lane == 0) {
            base = atomicAdd(&totals->n_list, (unsigned long long)cnt);
            ci = atomicAdd(narrow_class ? &totals->n_chunks_narrow : &totals->n_chunks, 1ull);
            if (narrow_class) atomicAdd(&totals->n_narrow_listed, (unsigned long long)cnt);
        }
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        ci = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(ci >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ci);
        if (base + cnt <= list_cap && ci < chunks_cap) {
            if (narrow_class) { for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) list[base + i] = st[NN_STAGE - 1 - i]; }
            else { for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) list[base + i] = i < fill ? st[i] : st[NN_STAGE - 1 - (i - fill)]; }
            if (lane == 0) { NNChunk ch; ch.slot = x; ch.count = cnt; ch.begin = base; chunks[(narrow_class ? chunks_cap : 0ull) + ci] = ch; }
        } else if (lane == 0) atomicOr(&totals->overflow, 1ull);
        if (narrow_class || merged) fill_n = 0;
        if (!narrow_class) fill = 0;
    };
#ifndef ISOCON_SURV_U
#define ISOCON_SURV_U 4
#endif
    // batches of 256 row positions (nn_surv_core.hpp) per iteration: their loads are independent.  Four: 0.84 ms at C3 against 0.87 with two and
    // 0.90 with eight; asking for the next iteration's loads ahead of the tests: 0.89 - 0.90 (profiles/surv_ab.txt; all before the stores were slimmed to 0.79)
    constexpr int U = ISOCON_SURV_U;
    const uint32_t q_block = Q.block();
    const uint32_t role_mask = (x_isq ? 1u << 21 : 0u) | (x_ist ? 1u << 22 : 0u);          // the role bits of a partner that make a direction of the pair
    // Q.entry() modulo 2^32 (entries are below 2^30)
    auto entry_of = [&](uint32_t s) { return Q.begin + (s >> Q.block_log2) * Q.stride + (s & (q_block - 1u)); };
    // the kept pairs of a batch into the staging buffer, by their keep masks; word(b): the list word of the lane's pair b
    auto stage_batch = [&](const uint64_t (&am)[SURV_PER_LANE], const uint64_t (&an)[SURV_PER_LANE], auto word) {
        fill = (uint32_t)__builtin_amdgcn_readfirstlane((int)fill);          // (wave-uniform, and the compiler should know it)
        fill_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)fill_n);
        surv_batch(am, an, fill, fill_n, NN_LIST_CHUNK,
                   [&](uint64_t lanes, uint32_t off_a, uint32_t off_n) {
                       if (surv_lane_bit(lanes, lane) == 0) return;
                       uint32_t at_a = off_a + surv_rank(am, lane), at_n = (uint32_t)NN_STAGE - 1u - (off_n + surv_rank(an, lane));
#pragma unroll
                       for (int b = 0; b < SURV_PER_LANE; ++b) {
                           const uint32_t ka = surv_lane_bit(am[b], lane), kn = surv_lane_bit(an[b], lane);
                           if (ka | kn) st[ka ? at_a : at_n] = word(b);
                           at_a += ka;
                           at_n -= kn;
                       }
                   },
                   [&](bool narrow_class) { emit_chunk(narrow_class); });          // the buffer is full: its larger class leaves (>= half a chunk)
    };
    // (the side is a compile-time constant of the loop body: own row = contiguous partners, transposed row = partners through the slot map)
    auto scan_side = [&](auto side_tag) {
        constexpr int side = decltype(side_tag)::value;
        const uint32_t len = side == 0 ? up_len : dn_len;
        const uint8_t *row = side == 0 ? B.lb + up_off : B.lbT + dn_off;
        const uint32_t tail = (len - 1u) & ~3u;          // where the lanes behind the row's end read (all their positions are masked)
        auto load_batches = [&](uint32_t c0, uint32_t (&lbv)[U], NNMeta4 (&my)[U]) {
            // lane l: the positions e0 .. e0 + 3.  Their four bounds are one dword at any byte address (a row's storage is padded to 16-byte
            // pieces and both matrices end with 16 spare bytes: nn_bounds.inc), their four meta words one 16-byte load at a dword address
            // (meta has three words of padding) wherever the partners are consecutive entries.
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * u + 4u * (uint32_t)lane;
                const uint32_t ec = e0 < len ? e0 : tail;
                __builtin_memcpy(&lbv[u], row + ec, 4);
                if (side == 0) my[u] = *reinterpret_cast<const NNMeta4 *>(meta + (x + 1u + ec));
                else {
                    // four slots are four consecutive entries inside one block of the map (or when the map's blocks touch)
                    const uint32_t s0 = dn_slo + ec;
                    const bool apart = Q.stride != q_block && (s0 & (q_block - 1u)) + 3u >= q_block;
                    if (__builtin_amdgcn_ballot_w64(apart) == 0) my[u] = *reinterpret_cast<const NNMeta4 *>(meta + entry_of(s0));
                    else {
#pragma unroll
                        for (int b = 0; b < SURV_PER_LANE; ++b) my[u][b] = meta[entry_of(dn_slo + (ec + b < len ? ec + b : len - 1u))];
                    }
                }
            }
        };
        auto scan_batches = [&](uint32_t c0, const uint32_t (&lbv)[U], const NNMeta4 (&my)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (c0 + (uint32_t)SURV_BATCH * u >= len) break;                        // wave-uniform
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * u + 4u * (uint32_t)lane;
                uint64_t am[SURV_PER_LANE], an[SURV_PER_LANE], aw[SURV_PER_LANE];          // keep masks: 64-row class, 32-row class, pairs that leave for their threshold
#pragma unroll
                for (int b = 0; b < SURV_PER_LANE; ++b) {
                    const uint32_t myb = my[u][b];
                    const SurvTest t = surv_test(e0 + b < len, x_isq, x_ist, (myb & (1u << 22)) != 0, (myb & (1u << 21)) != 0, kx0, nn_meta_thr(myb), P.kcap, m, (int32_t)nn_meta_len(myb),
                                                 (lbv[u] >> (8 * b)) & 0xffu, sx, nn_meta_score(myb), side, class_mode);
                    if (side == 0) { filtered += t.cand && !t.accept ? 1u : 0u; kept += t.accept ? 1u : 0u; }          // (per lane: summed once per entry)
                    // class mode +1: the pairs with a threshold above the 32-row form's go straight to the pair arrays
                    aw[b] = __builtin_amdgcn_ballot_w64(t.wide);
                    am[b] = __builtin_amdgcn_ballot_w64(t.keep && !t.to_narrow);
                    an[b] = __builtin_amdgcn_ballot_w64(t.to_narrow);
                }
                // (what a kept pair needs beyond its mask bit is made where it is stored: most batches keep nothing)
                // the list word of pair b: partner | x queries y << 30 | y queries x << 31 (a kept pair is in range: its role bits are the meta word's)
                const auto word = [&](int b) {
                    const uint32_t y = side == 0 ? x + 1u + e0 + (uint32_t)b : entry_of(dn_slo + e0 + (uint32_t)b);
                    return y | (my[u][b] & role_mask) << 9;
                };
                if (class_mode > 0) {                                        // wave-uniform
                    const uint32_t cw = surv_count(aw, ~(uint64_t)0);
                    if (cw != 0) {
                        unsigned long long wbase = 0;
                        if (lane == 0) {
                            wbase = atomicAdd(&totals->n_small, (unsigned long long)cw);
                            atomicAdd(&totals->n_wide_pairs, (unsigned long long)cw);
                            if (wbase + cw > small_cap) { atomicOr(&totals->overflow, 1ull); wbase = ~0ull; }
                        }
                        wbase = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(wbase >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wbase);
                        if (wbase != ~0ull) {
                            unsigned long long at = wbase + surv_rank(aw, lane);
#pragma unroll
                            for (int b = 0; b < SURV_PER_LANE; ++b) {
                                const uint32_t kw = surv_lane_bit(aw[b], lane);
                                if (kw) { pa[at] = x; pb[at] = word(b) & 0x3fffffffu; }
                                at += kw;
                            }
                        }
                    }
                }
                stage_batch(am, an, word);
            }
        };
        for (uint32_t c0 = 0; c0 < len; c0 += SURV_BATCH * U) {
            uint32_t lbv[U];
            NNMeta4 my[U];
            load_batches(c0, lbv, my);
            scan_batches(c0, lbv, my);
        }
    };
    // The same scan with the test on a lane's four pairs at once (nn_surv_core.hpp surv_test4): the partners' items come from the three
    // arrays of NNSurvSide, the keep masks as a bit per byte, and the ballots are only formed for a batch that keeps a pair at all.
    // Iterations whose U batches lie inside the row (full_tag) address by lane alone and mask nothing.
    uint32_t ncand_p = 0, kept_p = 0;          // candidates / accepted pairs of side 0 (per lane)
    auto scan_side_packed = [&](auto side_tag) {
        constexpr int side = decltype(side_tag)::value;
        const uint32_t len = side == 0 ? up_len : dn_len;
        const uint8_t *row = side == 0 ? B.lb + up_off : B.lbT + dn_off;
        const uint32_t tail = (len - 1u) & ~3u;
        const SurvX X = surv_x(x_isq, x_ist, kx0, P.kcap, m, sx, side, class_mode);
        const bool blocks_apart = side != 0 && Q.stride != q_block;          // (wave-uniform) consecutive slots need not be consecutive entries
        auto iteration = [&](uint32_t c0, auto full_tag) {
            constexpr bool full = decltype(full_tag)::value;
            uint32_t lbv[U], role[U], len7[U];
            uint2 sc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * u + 4u * (uint32_t)lane;
                const uint32_t ec = full || e0 < len ? e0 : tail;
                __builtin_memcpy(&lbv[u], row + ec, 4);
                const uint32_t y0 = side == 0 ? x + 1u + ec : entry_of(dn_slo + ec);
                const bool apart = blocks_apart && ((dn_slo + ec) & (q_block - 1u)) + 3u >= q_block;
                if (!blocks_apart || __builtin_amdgcn_ballot_w64(apart) == 0) {
                    __builtin_memcpy(&role[u], A.role + y0, 4);
                    __builtin_memcpy(&len7[u], A.len7 + y0, 4);
                    __builtin_memcpy(&sc[u], A.score + y0, 8);
                } else {
                    // a lane's four slots cross a block of the map: their items one by one (the slots behind the row's end read its last one)
                    role[u] = len7[u] = 0u;
                    sc[u] = make_uint2(0u, 0u);
#pragma unroll
                    for (int b = 0; b < SURV_PER_LANE; ++b) {
                        const uint32_t y = entry_of(dn_slo + (ec + b < len ? ec + b : len - 1u));
                        role[u] |= (uint32_t)A.role[y] << (8 * b);
                        len7[u] |= (uint32_t)A.len7[y] << (8 * b);
                        if (b < 2) sc[u].x |= (uint32_t)A.score[y] << (16 * b);
                        else sc[u].y |= (uint32_t)A.score[y] << (16 * (b - 2));
                    }
                }
            }
            // (a batch behind the row's end has no position inside it: it tests nothing true and keeps nothing)
            uint32_t keep[U], any = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * u + 4u * (uint32_t)lane;
                if (!full) role[u] &= surv_inr_bytes((int32_t)len - (int32_t)e0);          // (e0 and len are below 2^31)
                uint32_t cand, accept;
                surv_test4<side>(X, lbv[u], role[u], len7[u], sc[u].x, sc[u].y, cand, accept, keep[u]);
                if (side == 0) { ncand_p += (uint32_t)__popc(cand); kept_p += (uint32_t)__popc(accept); }
                any |= keep[u];
            }
            if (__builtin_amdgcn_ballot_w64(any != 0u) == 0) return;                             // wave-uniform: most iterations keep nothing
            // the ballots and the stores of the batches that keep a pair, one batch after the other (one copy of the code)
#pragma unroll 1
            for (int u = 0; u < U; ++u) {
                uint32_t keep_u = keep[0], role_u = role[0];
#pragma unroll
                for (int v = 1; v < U; ++v) { keep_u = u == v ? keep[v] : keep_u; role_u = u == v ? role[v] : role_u; }
                if (__builtin_amdgcn_ballot_w64(keep_u != 0u) == 0) continue;
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * (uint32_t)u + 4u * (uint32_t)lane;
                const uint32_t kn = keep_u & surv_narrow4(X, role_u), ka = keep_u & ~kn;
                uint64_t am[SURV_PER_LANE], an[SURV_PER_LANE];
#pragma unroll
                for (int b = 0; b < SURV_PER_LANE; ++b) {
                    am[b] = __builtin_amdgcn_ballot_w64((ka & (0x80u << (8 * b))) != 0u);
                    an[b] = __builtin_amdgcn_ballot_w64((kn & (0x80u << (8 * b))) != 0u);
                }
                // the list word of pair b (as above): the partner is a target -> x queries y, the partner queries (its b is not 0) -> y queries x
                const auto word = [&](int b) {
                    const uint32_t y = side == 0 ? x + 1u + e0 + (uint32_t)b : entry_of(dn_slo + e0 + (uint32_t)b);
                    const uint32_t rb = role_u >> (8 * b);
                    return y | (x_isq && (rb & 0x80u) ? 1u << 30 : 0u) | (x_ist && (rb & 0x7fu) ? 1u << 31 : 0u);
                };
                stage_batch(am, an, word);
            }
        };
        uint32_t c0 = 0;
        for (; c0 + (uint32_t)(SURV_BATCH * U) <= len; c0 += SURV_BATCH * U) iteration(c0, std::true_type());
        if (c0 < len) iteration(c0, std::false_type());
    };
    // (the host instantiates the packed form where every threshold + 1 fits seven bits and there is no third class: nn_surv_packed)
    if constexpr (PACKED) {
        scan_side_packed(std::integral_constant<int, 0>());
        scan_side_packed(std::integral_constant<int, 1>());
        filtered += ncand_p - kept_p;
        kept += kept_p;
    } else {
        scan_side(std::integral_constant<int, 0>());
        scan_side(std::integral_constant<int, 1>());
    }
    // the end of the entry's pairs: a class with enough pairs leaves as a chunk of its own; too few of the 32-row class join the 64-row
    // class (its kernel takes any threshold) before that class is judged
    if (fill_n >= list_min) emit_chunk(true);
    if (fill + fill_n >= list_min) emit_chunk(false, true);
    // what is left of both classes goes to the pair arrays (the pair-per-lane kernel takes any threshold)
    const uint32_t rest = fill + fill_n;
    // what is left goes to the pair arrays: one allocation per workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { filtered += __shfl_xor(filtered, o, 64); kept += __shfl_xor(kept, o, 64); }          // (counted per lane in the scan)
    // ... but for the pairs the seed pass has settled (NNSeedKnown): round t of a lane = item 64 t + lane, bit t of its mask = settled
    static_assert(NN_STAGE <= 64 * 64, "one mask bit per round of the staged pairs");
    const auto item = [&](uint32_t i) { return (i < fill ? st[i] : st[NN_STAGE - 1 - (i - fill)]) & 0x3fffffffu; };
    uint64_t settled_rounds = 0;
    uint32_t n_known = 0;          // (wave-uniform)
    if (K.known != nullptr) {
        for (uint32_t i0 = 0, t = 0; i0 < rest; i0 += 64, ++t) {
            const uint32_t i = i0 + (uint32_t)lane;
            const bool settled = i < rest && nn_seed_known(K.known, x, item(i));
            n_known += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(settled));
            if (settled) settled_rounds |= (uint64_t)1 << t;
        }
    }
    const uint32_t n_out = K.drop ? rest - n_known : rest;
    if (lane == 0) { s_small[wave] = n_out; s_filtered[wave] = filtered; s_kept[wave] = kept; s_known[wave] = n_known; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0, fsum = 0, ksum = 0, nsum = 0;
        for (int w = 0; w < NN_SURV_WAVES; ++w) { tot += s_small[w]; fsum += s_filtered[w]; ksum += s_kept[w]; nsum += s_known[w]; }
        unsigned long long base = 0;
        if (tot) {
            base = atomicAdd(&totals->n_small, (unsigned long long)tot);
            if (base + tot > small_cap) { atomicOr(&totals->overflow, 1ull); base = ~0ull; }
        }
        s_base = base;
        if (fsum) atomicAdd(&totals->n_filtered, (unsigned long long)fsum);
        if (ksum) atomicAdd(&totals->n_pairs, (unsigned long long)ksum);
        if (nsum) atomicAdd(&totals->n_seed_known, (unsigned long long)nsum);
    }
    __syncthreads();
    if (n_out && s_base != ~0ull) {
        unsigned long long base = s_base;
        for (int w = 0; w < wave; ++w) base += s_small[w];
        if (n_out == rest) { for (uint32_t i = (uint32_t)lane; i < rest; i += 64) { pa[base + i] = x; pb[base + i] = item(i); } }
        else {
            // the pairs that stay, dense: a round's survivors behind those of the rounds before
            const uint64_t below = ((uint64_t)1 << lane) - 1;
            for (uint32_t i0 = 0, t = 0; i0 < rest; i0 += 64, ++t) {
                const uint32_t i = i0 + (uint32_t)lane;
                const bool stays = i < rest && ((settled_rounds >> t) & 1u) == 0;
                const uint64_t sm = __builtin_amdgcn_ballot_w64(stays);
                if (stays) { const unsigned long long at = base + (unsigned long long)__popcll(sm & below); pa[at] = x; pb[at] = item(i); }
                base += (unsigned long long)__popcll(sm);
            }
        }
    }
}

// Largest chunks first (16 size classes, one workgroup): the table launch does not end with a few long workgroups (10.9 -> 10.4 ms at C3).
__global__ __launch_bounds__(1024) void k_nn_sort_chunks(const NNChunk *__restrict__ in, uint32_t n, NNChunk *__restrict__ out)
{
    __shared__ uint32_t hist[16], cursor[16];
    if (threadIdx.x < 16) hist[threadIdx.x] = 0;
    __syncthreads();
    auto cls = [](uint32_t count) { const uint32_t c = count / (NN_LIST_CHUNK / 16 + 1); return 15u - (c < 15u ? c : 15u); };
    for (uint32_t i = threadIdx.x; i < n; i += 1024) atomicAdd(&hist[cls(in[i].count)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t a = 0; for (int b = 0; b < 16; ++b) { cursor[b] = a; a += hist[b]; } }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 1024) { const NNChunk c = in[i]; out[atomicAdd(&cursor[cls(c.count)], 1u)] = c; }
}

}  // namespace isocon
