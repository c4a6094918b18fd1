// msa.hpp -- consensus correction of the partitions of a correction step (SURVEY.md 8(f) rows f1 + f3): their multi-alignment matrices built
// ON THE DEVICE from the CIGAR ops of the (centre, member) alignments and the packed store, then column statistics, per-read correction and
// gap stripping.  One kernel per step, all of them on a batch of partitions (MsaBatch); a single partition is a batch of one.
//
// The matrix is what the reference's modules/functions.py:543-588 (create_multialignment_matrix), :598-631 (position_query_to_alignment)
// and :679-767 (create_multialignment_format_NEW) assemble from the gapped strings of sw_align_sequences.  The gapped strings never exist
// here: an alignment is its run-length ops (isocon_sg_trace_batch; ~50 per pair at 2.5 kb), the bases come from the store's bit-planes.
// Layout (the reference's): in front of every centre base t and behind the last one sits a slot of insertion columns -- 1 column, or
// longest + 2 where some member inserts 2 or more characters (functions.py:722-731) -- followed by the base column of t.
//   k_msa_ops_scan     one thread per row: walks the row's ops, atomicMax of the insertion length per slot;
//   k_msa_layout       one workgroup per partition: slot widths and the exclusive prefix sums that give every slot's first column;
//   k_msa_fill         one wave per row: writes the row (the matrix is pre-filled with '-'); single-character insertions go to their
//                      slot's column, the insertions of WIDE slots are only listed (row, slot, position in the member, length, first bases,
//                      partition): where they sit inside the padded longest insertion is decided by get_best_solution (functions.py:635-676,
//                      string heuristics with an alignment tie).
// The placed builds (isocon_msa_build_ops_placed[_batch]) apply that rule on the device (msa_place_core.hpp) to every slot whose longest
// insertion has at most PLACE_MAX_LONGEST = 62 bases -- the padded insertion then fits the 64 lanes of a wave:
//   k_msa_wide_number  one thread per slot: numbers those slots, so that the per-slot keys scale with the wide slots and not with all slots;
//   k_msa_slot_rep     one thread per record, two passes: the slot's representative -- the smallest of its longest insertions -- as the
//                      atomicMin of big-endian 2-bit keys (bases 0 .. 31, then bases 32 .. 61 among the records that hold the first
//                      minimum); the first pass also copies the records of the slots it does NOT place (longest > 62: all of them, the host
//                      picks the representative from what it is handed) into a second list, one atomic per wave;
//   k_msa_place        one wave per record: substring test, DP by anti-diagonals + backtrack, best offset; writes the slot's columns of the row.
// The record list lives on the device, sized by the host from the code-3 ops (an upper bound); the result does not depend on its order,
// duplicates are computed again.  The existing builds hand ALL records to the host, whose placements come back as patches (k_msa_patch);
// after a placed build the patches are those of the left-over records only.
// ops: len << 4 | code, code 0 '=', 1 'X', 2 'I' (centre base against a gap of the member), 3 'D' (member bases the centre lacks:
// an insertion into the slot in front of the next centre base); the centre is the QUERY of its alignments (isocon_get_candidates.py:47).
//
// The correction is the reference's modules/correction_module.py:260-446 on those matrices:
//   k_msa_col_counts / k_msa_col_finish: per column the weighted counts of A, C, G, T, '-' (position frequency matrix, functions.py:526-536),
//                      the majority symbol (first maximum in that order), whether it is unique, and the partition's totals of the three
//                      error classes over the unambiguous columns (correction_module.py:296-307);
//   k_msa_row_correct  one wavefront per read: its correctable positions (unambiguous majority differs), their frequency
//                      own_count / class_total in double precision, the ceil(n/2)-th smallest frequency, and the replacement of every
//                      position at or below it by the majority symbol (:329-402);
//   k_msa_row_lengths / k_msa_strip: the corrected rows without their gap symbols, packed.
// Byte-matrix work, HBM-bound: the matrix is read three times and written once.
//
// Why a batch: the reference's correct_strings (correction_module.py:12-75) loops over the partitions (a Pool task each); later
// correction steps of a run have hundreds to thousands of small partitions, and one build + correct call pair per partition is ~20 host
// synchronisations each (2 751 call pairs over the ten steps of the 50 000-read set: 1.3 s).  So a row knows its partition (part_of_row)
// and a partition its pieces of the concatenated arrays: slots (insertion-slot arrays, len(centre) + 1 entries), columns (ncols entries)
// and matrix cells.
#pragma once
#include "common.hpp"
#include "msa_place_core.hpp"

namespace isocon {

struct MsaBatch {
    const uint32_t *part_of_row;          // [n_rows]
    const uint32_t *first_row;            // [n_parts + 1]: rows of partition p = first_row[p] .. first_row[p + 1]; the first is its centre
    const uint32_t *Lm;                   // [n_parts] length of the centre
    const uint32_t *slot_base;            // [n_parts + 1] offset of the partition's slot arrays (longest, width, col_slot)
    const uint32_t *ncols;                // [n_parts] columns of the partition's matrix (after k_msa_layout)
    const unsigned long long *m_off;      // [n_parts + 1] first cell of the partition's matrix
    const uint32_t *col_base;             // [n_parts + 1] offset of the partition's column arrays (counts, maj, flags)
    uint32_t n_parts, n_rows;
};

__device__ __forceinline__ uint8_t msa_base_char(const DevStore &S, uint32_t id, uint32_t pos)
{
    const size_t w = ((size_t)(pos >> 6) * S.n + id) * 2;
    const uint32_t sh = pos & 63u;
    const uint32_t code = (uint32_t)((S.planes[w] >> sh) & 1ull) | ((uint32_t)((S.planes[w + 1] >> sh) & 1ull) << 1);
    return (uint8_t)("ACGT"[code]);
}

__device__ __forceinline__ int msa_sym(uint8_t c)      // A C G T - -> 0..4
{
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}

// longest[slot_base[p] + t] = longest insertion any row of partition p has in slot t (t = 0 .. Lm); bad[0] != 0 if a row's ops do not spell
// the centre / the member
__global__ __launch_bounds__(256) void k_msa_ops_scan(DevStore S, MsaBatch B, const uint32_t *__restrict__ row_ids, const uint32_t *__restrict__ ops,
                                                       const unsigned long long *__restrict__ ops_ptr, uint32_t *__restrict__ longest, uint32_t *__restrict__ bad)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= B.n_rows) return;
    const uint32_t p = B.part_of_row[r];
    if (r == B.first_row[p]) return;          // the centre itself: no ops, no insertions
    const uint32_t Lm = B.Lm[p];
    uint32_t *lg = longest + B.slot_base[p];
    uint32_t t = 0, sp = 0;
    for (unsigned long long k = ops_ptr[r]; k < ops_ptr[r + 1]; ++k) {
        const uint32_t op = ops[k], len = op >> 4, code = op & 15u;
        if (code == 3u) { if (t <= Lm) atomicMax(lg + t, len); sp += len; }
        else { t += len; if (code != 2u) sp += len; }
    }
    if (t != Lm || sp != (uint32_t)S.lens[row_ids[r]]) atomicOr(bad, 1u);
}

// width[t] = 1 or longest + 2; col_slot[t] = first column of slot t (the base column of t follows the slot); ncols_out[p] = the partition's
// columns.  One workgroup of 1024 threads per partition.
__global__ __launch_bounds__(1024) void k_msa_layout(MsaBatch B, const uint32_t *__restrict__ longest, uint32_t *__restrict__ width, uint32_t *__restrict__ col_slot,
                                                      uint32_t *__restrict__ ncols_out)
{
    __shared__ unsigned long long wave_sums[16];
    __shared__ unsigned long long carry;
    const uint32_t p = blockIdx.x;
    const uint32_t Lm = B.Lm[p], sb = B.slot_base[p];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base <= Lm; base += 1024u) {
        const uint32_t t = base + threadIdx.x;
        uint32_t w = 0;
        if (t <= Lm) {
            const uint32_t lg = longest[sb + t];
            w = lg > 1u ? lg + 2u : 1u;
            width[sb + t] = w;
        }
        unsigned long long total = 0;
        const unsigned long long step = t <= Lm ? (unsigned long long)w + (t < Lm ? 1ull : 0ull) : 0ull;      // slot + its base column (the last slot has none)
        const unsigned long long off = block_exscan_1024(step, wave_sums, &total);
        if (t <= Lm) col_slot[sb + t] = (uint32_t)(carry + off);
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) ncols_out[p] = (uint32_t)carry;
}

// One wave per row.  wide[8 i ..] = row (of the concatenation), slot, first position in the member, length, the 2-bit codes (A C G T = 0 1 2 3)
// of its first 32 bases (base j at bits 2 j of the 64-bit word lo | hi << 32), the partition, a spare word; wide_count: entries appended (may
// exceed wide_cap: the host then calls again with room).
__global__ __launch_bounds__(256) void k_msa_fill(DevStore S, MsaBatch B, const uint32_t *__restrict__ row_ids, const uint32_t *__restrict__ ops,
                                                   const unsigned long long *__restrict__ ops_ptr, const uint32_t *__restrict__ longest_all,
                                                   const uint32_t *__restrict__ width_all, const uint32_t *__restrict__ col_slot_all, uint8_t *__restrict__ M_all,
                                                   uint32_t *__restrict__ wide, unsigned long long wide_cap, unsigned long long *__restrict__ wide_count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 4u + (uint32_t)wave;
    if (r >= B.n_rows) return;
    const uint32_t p = B.part_of_row[r], r0 = B.first_row[p], Lm = B.Lm[p], sb = B.slot_base[p], n_cols = B.ncols[p];
    const uint32_t *longest = longest_all + sb, *width = width_all + sb, *col_slot = col_slot_all + sb;
    const uint32_t id = row_ids[r];
    uint8_t *row = M_all + B.m_off[p] + (size_t)(r - r0) * n_cols;
    if (r == r0) {          // the centre: its own bases in the base columns
        for (uint32_t t = (uint32_t)lane; t < Lm; t += 64u) row[col_slot[t] + width[t]] = msa_base_char(S, id, t);
        return;
    }
    // The row's ops, 64 at a time: every lane loads one (coalesced), a wave scan gives each op its slot and member position, and the ops are then
    // taken one by one from the lanes' registers -- no chain of dependent global loads (op k + 1 could not be requested before op k had arrived).
    uint32_t t = 0, sp = 0;
    const unsigned long long k_end = ops_ptr[r + 1];
    for (unsigned long long kb = ops_ptr[r]; kb < k_end; kb += 64ull) {
        const uint32_t n_here = (uint32_t)(k_end - kb < 64ull ? k_end - kb : 64ull);
        const uint32_t op_l = (uint32_t)lane < n_here ? ops[kb + (unsigned long long)lane] : 0u;
        const uint32_t len_l = op_l >> 4, code_l = op_l & 15u;
        uint32_t it = code_l == 3u ? 0u : len_l, is = code_l == 2u ? 0u : len_l;          // inclusive scans of the advances in slot / member position
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ot = (uint32_t)__shfl_up((int)it, d, 64), os = (uint32_t)__shfl_up((int)is, d, 64);
            if (lane >= d) { it += ot; is += os; }
        }
        const uint32_t t_l = t + it - (code_l == 3u ? 0u : len_l), sp_l = sp + is - (code_l == 2u ? 0u : len_l);
        // Insertions at wide slots are only LISTED (their place inside the padded longest insertion is decided by k_msa_place, or on the host): every lane files
        // its own op's record, ONE atomic per batch reserves the records (one atomic per record -- 6 10^5 on one address at C3 -- was what the
        // kernel's 3.7 ms were: same-address atomics serialise in L2).
        {
            // (a malformed op stream -- an op that runs past the member row -- ends the row at that op below: the records of the ops behind it
            // are not listed either: the lanes in front of the first op that fails the bound)
            const unsigned long long bad = __ballot((uint32_t)lane < n_here && t_l + (code_l == 3u ? 0u : len_l) > Lm);
            const bool before_bad = bad == 0ull || (uint32_t)lane < (uint32_t)__builtin_ctzll(bad);
            const bool wide_l = before_bad && (uint32_t)lane < n_here && code_l == 3u && t_l <= Lm && longest[t_l] > 1u;
            const unsigned long long wm = __ballot(wide_l);
            if (wm != 0ull) {
                unsigned long long at0 = 0;
                if (lane == 0) at0 = atomicAdd(wide_count, (unsigned long long)__popcll(wm));
                at0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(at0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at0);
                const unsigned long long at = at0 + (unsigned long long)__popcll(wm & (((unsigned long long)1 << lane) - 1ull));
                if (wide_l && at < wide_cap) {
                    unsigned long long codes = 0;
                    for (uint32_t jj = 0; jj < len_l && jj < 32u; ++jj) {
                        const size_t w = ((size_t)((sp_l + jj) >> 6) * S.n + id) * 2;
                        const uint32_t sh = (sp_l + jj) & 63u;
                        codes |= (((S.planes[w] >> sh) & 1ull) | (((S.planes[w + 1] >> sh) & 1ull) << 1)) << (2u * jj);
                    }
                    uint32_t *e = wide + 8 * at;
                    e[0] = r; e[1] = t_l; e[2] = sp_l; e[3] = len_l; e[4] = (uint32_t)codes; e[5] = (uint32_t)(codes >> 32); e[6] = p; e[7] = 0u;
                }
            }
        }
        for (uint32_t j = 0; j < n_here; ++j) {
            const uint32_t op = (uint32_t)__builtin_amdgcn_readlane((int)op_l, (int)j), len = op >> 4, code = op & 15u;
            const uint32_t tj = (uint32_t)__builtin_amdgcn_readlane((int)t_l, (int)j), spj = (uint32_t)__builtin_amdgcn_readlane((int)sp_l, (int)j);
            if (tj + (code == 3u ? 0u : len) > Lm) return;          // (ops that do not spell the centre were reported by k_msa_ops_scan)
            if (code == 3u) {
                if (longest[tj] <= 1u && lane == 0) row[col_slot[tj]] = msa_base_char(S, id, spj);          // (wide slots: listed above)
            } else {
                for (uint32_t i = (uint32_t)lane; i < len; i += 64u)
                    row[col_slot[tj + i] + width[tj + i]] = code == 2u ? (uint8_t)'-' : msa_base_char(S, id, spj + i);
            }
        }
        t += (uint32_t)__shfl((int)it, 63, 64);
        sp += (uint32_t)__shfl((int)is, 63, 64);
    }
}

// ---- the wide-slot insertions placed on the device (msa_place_core.hpp) ---------------------------------------------------------------------

static constexpr uint32_t MSA_NO_WIDE = 0xffffffffu;          // wide_idx of a slot the device does not place (1 column, or longest > PLACE_MAX_LONGEST)

__device__ __forceinline__ uint32_t msa_base_code(const DevStore &S, uint32_t id, uint32_t pos)
{
    const size_t w = ((size_t)(pos >> 6) * S.n + id) * 2;
    const uint32_t sh = pos & 63u;
    return (uint32_t)((S.planes[w] >> sh) & 1ull) | ((uint32_t)((S.planes[w + 1] >> sh) & 1ull) << 1);
}

// 64 bases of sequence id from position pos on, one plane; a chunk outside the store reads as 0
__device__ __forceinline__ uint64_t msa_fetch64(const DevStore &S, uint32_t id, uint32_t plane, uint32_t pos)
{
    const uint32_t c = pos >> 6, sh = pos & 63u;
    const uint64_t w0 = c < S.nchunks ? S.planes[((size_t)c * S.n + id) * 2 + plane] : 0ull;
    if (!sh) return w0;
    const uint64_t w1 = c + 1u < S.nchunks ? S.planes[((size_t)(c + 1u) * S.n + id) * 2 + plane] : 0ull;
    return (w0 >> sh) | (w1 << (64u - sh));
}

// wide_idx[s] = the slot's number among the slots the device places (2 <= longest <= PLACE_MAX_LONGEST), in no particular order;
// *n_wide_slots (zeroed by the host) = how many there are
__global__ __launch_bounds__(256) void k_msa_wide_number(const uint32_t *__restrict__ longest, uint32_t n_slots, uint32_t *__restrict__ wide_idx, uint32_t *__restrict__ n_wide_slots)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long s = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool placed = s < n_slots && longest[s] > 1u && longest[s] <= (uint32_t)PLACE_MAX_LONGEST;
    const unsigned long long mask = __ballot(placed);
    uint32_t base = 0;
    if (mask != 0ull) {
        if (lane == 0) base = atomicAdd(n_wide_slots, (uint32_t)__popcll(mask));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    }
    if (s < n_slots) wide_idx[s] = placed ? base + (uint32_t)__popcll(mask & (((unsigned long long)1 << lane) - 1ull)) : MSA_NO_WIDE;
}

// One thread per record of `wide` (min(*wide_count, wide_cap) of them).  keys[2 x], keys[2 x + 1] (preset to PLACE_KEY_NONE) = the keys of
// the representative of placed slot x.  PASS 1: first key; and the records of the slots that are not placed go to left (8 words each, as in
// wide; *left_count may exceed left_cap).  PASS 2: second key, for slots with longest > 32.
template <int PASS>
__global__ __launch_bounds__(256) void k_msa_slot_rep(DevStore S, MsaBatch B, const uint32_t *__restrict__ row_ids, const uint32_t *__restrict__ longest_all,
                                                       const uint32_t *__restrict__ wide_idx_all, const uint32_t *__restrict__ wide, unsigned long long wide_cap,
                                                       const unsigned long long *__restrict__ wide_count, unsigned long long *__restrict__ keys,
                                                       uint32_t *__restrict__ left, unsigned long long left_cap, unsigned long long *__restrict__ left_count)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long n = *wide_count < wide_cap ? *wide_count : wide_cap;
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    const bool have = i < n;
    const uint32_t *e = wide + 8 * (have ? i : 0ull);
    uint32_t idx = MSA_NO_WIDE, lg = 0, len = 0;
    unsigned long long codes = 0;
    if (have) {
        const uint32_t sb = B.slot_base[e[6]];
        idx = wide_idx_all[sb + e[1]];
        lg = longest_all[sb + e[1]];
        len = e[3];
        codes = (unsigned long long)e[4] | ((unsigned long long)e[5] << 32);
    }
    if (PASS == 1) {
        const bool over = have && idx == MSA_NO_WIDE;
        const unsigned long long mask = __ballot(over);
        if (mask != 0ull) {
            unsigned long long at0 = 0;
            if (lane == 0) at0 = atomicAdd(left_count, (unsigned long long)__popcll(mask));
            at0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(at0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at0);
            const unsigned long long at = at0 + (unsigned long long)__popcll(mask & (((unsigned long long)1 << lane) - 1ull));
            if (over && at < left_cap)
                for (int k = 0; k < 8; ++k) left[8 * at + k] = e[k];
        }
        if (have && idx != MSA_NO_WIDE && len == lg) atomicMin(keys + 2 * (size_t)idx, (unsigned long long)place_key_of_codes(codes));
    } else {
        if (have && idx != MSA_NO_WIDE && len == lg && lg > 32u && place_key_of_codes(codes) == keys[2 * (size_t)idx]) {
            const uint32_t id = row_ids[e[0]], pos = e[2] + 32u;
            atomicMin(keys + 2 * (size_t)idx + 1, (unsigned long long)place_key_of_planes(msa_fetch64(S, id, 0, pos), msa_fetch64(S, id, 1, pos), (int)(len - 32u)));
        }
    }
}

// One wave per record, four per workgroup: the record's insertion q (its first 32 bases from the record, the rest from the store's planes)
// inside '-' + its slot's representative + '-' (from the slot's keys), written into the L = longest + 2 columns of the slot in the record's row.
// Everything that decides a branch is wave-uniform: the strings are words the whole wave shares (PlaceStr), each step's outcome a ballot or a
// wave maximum.  LDS: the DP bytes, PLACE_DP_BYTES per wave.
__global__ __launch_bounds__(256) void k_msa_place(DevStore S, MsaBatch B, const uint32_t *__restrict__ row_ids, const uint32_t *__restrict__ longest_all,
                                                    const uint32_t *__restrict__ col_slot_all, const uint32_t *__restrict__ wide_idx_all,
                                                    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ wide, unsigned long long wide_cap,
                                                    const unsigned long long *__restrict__ wide_count, uint8_t *__restrict__ M_all)
{
    __shared__ uint8_t s_D[4][PLACE_DP_BYTES];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long n = *wide_count < wide_cap ? *wide_count : wide_cap;
    const unsigned long long i = (unsigned long long)blockIdx.x * 4ull + wave;
    if (i >= n) return;
    const uint32_t *e = wide + 8 * i;
    const uint32_t r = e[0], t = e[1], sp = e[2], p = e[6];
    const int m = (int)e[3];
    const unsigned long long codes = (unsigned long long)e[4] | ((unsigned long long)e[5] << 32);
    const uint32_t sb = B.slot_base[p], idx = wide_idx_all[sb + t];
    if (idx == MSA_NO_WIDE) return;          // (a slot left to the host)
    const int lg = (int)longest_all[sb + t], L = lg + 2;
    if (m < 1 || m > lg || lg > PLACE_MAX_LONGEST) return;          // (cannot be: longest is the maximum over these very records)
    const unsigned long long k1 = keys[2 * (size_t)idx], k2 = keys[2 * (size_t)idx + 1];
    const uint32_t rc = lane < lg ? place_key_code(k1, k2, lane) : 0u;
    const PlaceStr mx = place_padded(__ballot((rc & 1u) != 0u), __ballot((rc & 2u) != 0u), lg);
    uint32_t qc = 0;
    if (lane < m) qc = lane < 32 ? (uint32_t)((codes >> (2 * lane)) & 3ull) : msa_base_code(S, row_ids[r], sp + (uint32_t)lane);
    PlaceStr q, o;
    q.v = place_low(m);
    q.b0 = __ballot((qc & 1u) != 0u);
    q.b1 = __ballot((qc & 2u) != 0u);
    const unsigned long long found = __ballot(lane <= L - m && place_eq(mx, q, lane) == q.v);
    if (found != 0ull) o = place_at(q, __builtin_ctzll(found));          // 1. substring: the first occurrence
    else {
        uint8_t *D = s_D[wave];
        uint32_t prev = 0, prev2 = 0, cur = 0;          // this lane's column j = lane + 1 on the two previous anti-diagonals
        const int j = lane + 1;
        for (int d = 2; d <= L + m; ++d) {
            const uint32_t left_in = (uint32_t)__shfl_up((int)prev, 1, 64), diag_in = (uint32_t)__shfl_up((int)prev2, 1, 64);
            const int ii = d - j;
            if (j <= m && ii >= 1 && ii <= L) {
                const uint32_t up = ii == 1 ? (uint32_t)j : prev;
                const uint32_t left = lane == 0 ? (uint32_t)ii : left_in;
                const uint32_t diag = lane == 0 ? (uint32_t)(ii - 1) : ii == 1 ? (uint32_t)(j - 1) : diag_in;
                cur = place_dp_value(up, left, diag, mx, q, ii, j);
                D[place_dp_index(ii, j)] = (uint8_t)cur;
            }
            prev2 = prev;
            prev = cur;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // (the backtrack reads what other lanes of the wave wrote)
        __builtin_amdgcn_wave_barrier();
        if (!place_thread(D, L, m, q, o)) {          // 2. threading, else 3. the offset with the most matches
            uint32_t key = lane <= L - m ? place_offset_key(mx, q, lane) : 0u;
            for (int s = 32; s > 0; s >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)key, s, 64); key = other > key ? other : key; }
            o = place_at(q, place_offset_of_key((uint32_t)__builtin_amdgcn_readfirstlane((int)key)));
        }
    }
    uint8_t *row = M_all + B.m_off[p] + (size_t)(r - B.first_row[p]) * B.ncols[p] + col_slot_all[sb + t];
    if (lane < L) row[lane] = place_char(o, lane);
}

// patches: bytes[ptr[i] .. ptr[i + 1]) go to row patch_row[i] (of the concatenation) from column patch_col[i] of its matrix on (one wave per patch)
__global__ __launch_bounds__(256) void k_msa_patch(uint8_t *__restrict__ M_all, MsaBatch B, const uint32_t *__restrict__ patch_row, const uint32_t *__restrict__ patch_col,
                                                    const uint32_t *__restrict__ patch_ptr, const uint8_t *__restrict__ bytes, uint32_t n_patches)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4u + (uint32_t)wave;
    if (i >= n_patches) return;
    const uint32_t r = patch_row[i], p = B.part_of_row[r];
    uint8_t *dst = M_all + B.m_off[p] + (size_t)(r - B.first_row[p]) * B.ncols[p] + patch_col[i];
    const uint32_t b = patch_ptr[i], e = patch_ptr[i + 1];
    for (uint32_t k = b + (uint32_t)lane; k < e; k += 64u) dst[k - b] = bytes[k];
}

// Column statistics in two launches (one thread per column walking ALL rows of its partition -- 11 000 at C3 -- took 6.2 ms with 110
// workgroups on the chip):
//   k_msa_col_counts   workgroup b = the 256 columns cbr[3b + 1] .. of partition cbr[3b], rows cbr[3b + 2] .. + MSA_ROWS_PER_WG (host-built table):
//                      per-column symbol counts of that row chunk, weighted by the rows' degrees, added to counts (zeroed by the host);
//                      counts[5 col_base[p] + s * ncols + col]
//   k_msa_col_finish   workgroup b = the 256 columns cb_col0[b] .. of partition cb_part[b]: maj[col] = majority symbol index, flags[col] bit 0 =
//                      unambiguous, class_tot[3 p ..] = the partition's error-class totals (ins, del, subs; zeroed by the host)
static constexpr uint32_t MSA_ROWS_PER_WG = 256;

__global__ __launch_bounds__(256) void k_msa_col_counts(const uint8_t *__restrict__ M_all, MsaBatch B, const uint32_t *__restrict__ cbr, const int32_t *__restrict__ degree,
                                                         int32_t *__restrict__ counts_all)
{
    const uint32_t p = cbr[3 * blockIdx.x], col = cbr[3 * blockIdx.x + 1] + threadIdx.x, row0 = cbr[3 * blockIdx.x + 2];
    const uint32_t ncols = B.ncols[p], r0 = B.first_row[p], nr = B.first_row[p + 1] - r0;
    if (col >= ncols) return;
    const uint32_t row1 = row0 + MSA_ROWS_PER_WG < nr ? row0 + MSA_ROWS_PER_WG : nr;
    const uint8_t *M = M_all + B.m_off[p];
    int32_t c[5] = {0, 0, 0, 0, 0};
#pragma unroll 8
    for (uint32_t r = row0; r < row1; ++r) {
        const int sidx = msa_sym(M[(size_t)r * ncols + col]);
        const int32_t d = degree[r0 + r];
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += sidx == k ? d : 0;
    }
    int32_t *counts = counts_all + (size_t)5 * B.col_base[p];
#pragma unroll
    for (int k = 0; k < 5; ++k) if (c[k]) atomicAdd(counts + (size_t)k * ncols + col, c[k]);
}

__global__ __launch_bounds__(256) void k_msa_col_finish(MsaBatch B, const uint32_t *__restrict__ cb_part, const uint32_t *__restrict__ cb_col0,
                                                         const int32_t *__restrict__ counts_all, uint8_t *__restrict__ maj_all,
                                                         uint8_t *__restrict__ flags_all, unsigned long long *__restrict__ class_tot_all)
{
    const uint32_t p = cb_part[blockIdx.x], col = cb_col0[blockIdx.x] + threadIdx.x;
    const uint32_t ncols = B.ncols[p];
    const int32_t *counts = counts_all + (size_t)5 * B.col_base[p];
    long long ci = 0, cd = 0, cs = 0;
    if (col < ncols) {
        int32_t c[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] = counts[(size_t)k * ncols + col];
        int best = 0, ties = 1;
#pragma unroll
        for (int k = 1; k < 5; ++k) {
            if (c[k] > c[best]) { best = k; ties = 1; }
            else if (c[k] == c[best]) ++ties;
        }
        int32_t tot = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) tot += c[k];
        maj_all[B.col_base[p] + col] = (uint8_t)best;
        flags_all[B.col_base[p] + col] = ties == 1 ? 1 : 0;
        if (ties == 1) {
            if (best == 4) ci = tot - c[4];
            else { cd = c[4]; cs = tot - c[best] - c[4]; }
        }
    }
    // block reduction of the three totals
    __shared__ long long red[3][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) { ci += __shfl_xor(ci, o, 64); cd += __shfl_xor(cd, o, 64); cs += __shfl_xor(cs, o, 64); }
    if (lane == 0) { red[0][wave] = ci; red[1][wave] = cd; red[2][wave] = cs; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const long long t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (t) atomicAdd(class_tot_all + (size_t)3 * p + threadIdx.x, (unsigned long long)t);
    }
}

// Correctable positions per row that k_msa_row_correct<CAP> keeps in LDS.  2 048: a workgroup of four rows takes 96 KB -- ONE workgroup per CU,
// one wave per SIMD, 4.2 ms for the 50 000 rows of C3 (25-60 candidates each).  1 024: 48 KB, three workgroups per CU; the batched entry point
// runs that one and hands a row with more (reads of > 8 kb at ONT error rates) back to its caller, who sends the row's partition through the
// single-partition entry points; those run 2 048 and then MSA_LIST_HBM for the rows that are left.
static constexpr int MSA_BATCH_CAND = 1024;
static constexpr int MSA_MAX_CAND = 2048;
static constexpr int MSA_LIST_HBM = 0;          // as CAP: the list in a global scratch row, as long as the row's matrix is wide

// list accessors: LDS directly; global scratch through device-scope atomics (lanes read what other lanes of the wave wrote)
template <bool GLOBAL> __device__ __forceinline__ void msa_put(double *fq, uint32_t *cl, uint32_t at, double f, uint32_t col)
{
    if (GLOBAL) {
        __hip_atomic_store((unsigned long long *)fq + at, (unsigned long long)__double_as_longlong(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(cl + at, col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else { fq[at] = f; cl[at] = col; }
}
template <bool GLOBAL> __device__ __forceinline__ double msa_freq(const double *fq, uint32_t i)
{
    if (GLOBAL) return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)fq + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    return fq[i];
}
template <bool GLOBAL> __device__ __forceinline__ uint32_t msa_col(const uint32_t *cl, uint32_t i)
{
    if (GLOBAL) return __hip_atomic_load(cl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return cl[i];
}

// One wavefront per row.  out row = corrected row; n_cand[r] = number of correctable positions.  CAP > 0: every row of the batch, its list in
// LDS; a row with more than CAP positions gets n_cand = -1 and is left to the caller.  CAP = MSA_LIST_HBM: the rows of `row_list` (n_list of
// them), their lists in g_freq / g_col (list_stride entries per listed row: at least the widest of their matrices).
template <int CAP>
__global__ __launch_bounds__(256) void k_msa_row_correct(const uint8_t *__restrict__ M_all, uint8_t *__restrict__ out_all, MsaBatch B, const int32_t *__restrict__ degree,
                                                          const int32_t *__restrict__ counts_all, const uint8_t *__restrict__ maj_all, const uint8_t *__restrict__ flags_all,
                                                          const unsigned long long *__restrict__ class_tot_all, int32_t *__restrict__ n_cand,
                                                          const uint32_t *__restrict__ row_list, uint32_t n_list, double *g_freq, uint32_t *g_col, uint32_t list_stride)
{
    constexpr bool GLOBAL = CAP == MSA_LIST_HBM;
    __shared__ double s_freq[GLOBAL ? 1 : 4][GLOBAL ? 1 : CAP];
    __shared__ uint32_t s_col[GLOBAL ? 1 : 4][GLOBAL ? 1 : CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t slot = blockIdx.x * 4 + wave;
    if (slot >= (GLOBAL ? n_list : B.n_rows)) return;
    const uint32_t r = GLOBAL ? row_list[slot] : slot;
    const uint32_t p = B.part_of_row[r], ncols = B.ncols[p];
    const uint32_t cap = GLOBAL ? ncols : (uint32_t)CAP;
    const size_t cell0 = B.m_off[p] + (size_t)(r - B.first_row[p]) * ncols;
    const uint8_t *row = M_all + cell0;
    uint8_t *orow = out_all + cell0;
    const int32_t *counts = counts_all + (size_t)5 * B.col_base[p];
    const uint8_t *maj = maj_all + B.col_base[p], *flags = flags_all + B.col_base[p];
    const unsigned long long *class_tot = class_tot_all + (size_t)3 * p;
    const char SYM[5] = {'A', 'C', 'G', 'T', '-'};
    const double d_ins = (double)(class_tot[0] > 0 ? class_tot[0] : 1ull);
    const double d_del = (double)(class_tot[1] > 0 ? class_tot[1] : 1ull);
    const double d_sub = (double)(class_tot[2] > 0 ? class_tot[2] : 1ull);
    const bool single = degree[r] == 1;
    double *fq = GLOBAL ? g_freq + (size_t)slot * list_stride : s_freq[wave];
    uint32_t *cl = GLOBAL ? g_col + (size_t)slot * list_stride : s_col[wave];
    uint32_t n = 0;                 // candidates so far (wave-uniform)
    bool overflow = false;
    for (uint32_t c0 = 0; c0 < ncols; c0 += 64) {
        const uint32_t col = c0 + lane;
        uint8_t v = '-';
        bool cand = false;
        if (col < ncols) {
            v = row[col];
            orow[col] = v;
            cand = single && flags[col] && v != (uint8_t)SYM[maj[col]];
        }
        const unsigned long long mask = __ballot(cand);
        if (mask) {
            const uint32_t at = n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (cand && at < cap) {
                const int mj = maj[col];
                const double own = (double)counts[(size_t)msa_sym(v) * ncols + col];
                msa_put<GLOBAL>(fq, cl, at, own / (mj == 4 ? d_ins : (v == '-' ? d_del : d_sub)), col);
            }
            n += (uint32_t)__popcll(mask);
            if (n > cap) overflow = true;
        }
    }
    if (overflow) { if (lane == 0) n_cand[r] = -1; return; }
    if (lane == 0) n_cand[r] = (int32_t)n;
    if (n == 0) return;
    if (GLOBAL) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // threshold = k-th smallest frequency, k = ceil(n / 2): the value f with  #{< f} < k <= #{<= f}
    const uint32_t k = (n + 1) / 2;
    double thr = 0.0;
    bool have = false;
    for (uint32_t i0 = 0; i0 < n && !have; i0 += 64) {
        const uint32_t i = i0 + lane;
        bool mine = false;
        double f = 0.0;
        if (i < n) {
            f = msa_freq<GLOBAL>(fq, i);
            uint32_t lt = 0, le = 0;
            for (uint32_t j = 0; j < n; ++j) { const double g = msa_freq<GLOBAL>(fq, j); lt += g < f; le += g <= f; }
            mine = lt < k && k <= le;
        }
        const unsigned long long m2 = __ballot(mine);
        if (m2) {
            const int src = __ffsll((long long)m2) - 1;
            thr = __shfl(f, src, 64);
            have = true;
        }
    }
    for (uint32_t i = lane; i < n; i += 64)
        if (msa_freq<GLOBAL>(fq, i) <= thr) { const uint32_t c = msa_col<GLOBAL>(cl, i); orow[c] = (uint8_t)SYM[maj[c]]; }
}

__global__ __launch_bounds__(256) void k_msa_row_lengths(const uint8_t *__restrict__ rows_all, MsaBatch B, uint32_t *__restrict__ len)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 4 + wave;
    if (r >= B.n_rows) return;
    const uint32_t p = B.part_of_row[r], ncols = B.ncols[p];
    const uint8_t *row = rows_all + B.m_off[p] + (size_t)(r - B.first_row[p]) * ncols;
    uint32_t c = 0;
    for (uint32_t col = lane; col < ncols; col += 64) c += row[col] != '-';
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) len[r] = c;
}

__global__ __launch_bounds__(256) void k_msa_strip(const uint8_t *__restrict__ rows_all, MsaBatch B, const uint64_t *__restrict__ off, uint8_t *__restrict__ packed)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 4 + wave;
    if (r >= B.n_rows) return;
    const uint32_t p = B.part_of_row[r], ncols = B.ncols[p];
    const uint8_t *row = rows_all + B.m_off[p] + (size_t)(r - B.first_row[p]) * ncols;
    uint8_t *dst = packed + off[r];
    uint32_t at = 0;
    for (uint32_t c0 = 0; c0 < ncols; c0 += 64) {
        const uint32_t col = c0 + lane;
        const uint8_t v = col < ncols ? row[col] : (uint8_t)'-';
        const bool keep = v != '-';
        const unsigned long long mask = __ballot(keep);
        if (keep) dst[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = v;
        at += (uint32_t)__popcll(mask);
    }
}

}  // namespace isocon
