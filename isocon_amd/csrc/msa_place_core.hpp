// msa_place_core.hpp -- where an insertion sits inside the wide slot of a multi-alignment matrix (k_msa_slot_rep / k_msa_place, msa.hpp):
// functions.get_best_solution (the reference's modules/functions.py:635-676 with min_ed :771-799 and functions.nw_path_cigar where the
// reference calls edlib) on bit words.  The host statements of the same rule: functions.get_best_solution and cpy/_pyhelp.c best_solution.
//
// One record: mx[0 .. L) = '-' + the slot's representative longest insertion + '-' (L = longest + 2 <= PLACE_MAX_L = 64) and the record's
// insertion q[0 .. m) over ACGT, 1 <= m <= longest.  Result: L columns, each '-' or a base of q.
//   1. substring  the first occurrence of q in mx: q there, gaps elsewhere;
//   2. threading  otherwise the unit-cost global DP of mx (rows) against q (columns), backtracked from the end with the preference
//                 mx alone > q alone > diagonal: a step in mx alone is '-', a diagonal step the character of q, the first step in q alone
//                 abandons the threading;
//   3. offset     then the offset p in [0, L - m] with the most positions q[t] == mx[p + t], the first maximum, counted only with at least
//                 one match: q sits at p if p > 0 and at column 0 -- on the pad column -- otherwise.
// The pads of mx are ordinary characters that match nothing: ('-AA-', 'C') -> 'C---'.
//
// A string of up to 64 characters over A C G T - is three 64-bit words (PlaceStr): bit t of v says that column t holds a base, bits t of
// b0 and b1 are its 2-bit code (A C G T = 0 1 2 3, the store's planes).  mx and q of a record are the same for all lanes of its wave, so
// these words are wave-uniform; q[t] == mx[p + t] for all t at once is a shift and two XORs (place_eq), steps 1 and 3 are one such word per
// offset -- a lane each -- and the result is a PlaceStr again.  Step 2 is the DP by anti-diagonals, lane l on column j = l + 1 with the
// two previous diagonals in registers (place_dp_value; its neighbours' values come from lane l - 1), every cell also stored as a byte
// (values <= 64) for the backtrack; row 0 and column 0 are not stored (D[i][0] = i, D[0][j] = j): PLACE_DP_BYTES = 64 * 62.  The backtrack
// (place_thread) reads wave-uniform addresses and builds the result in scalar words.
//
// The representative of a slot -- the smallest of its longest insertions as strings, A < C < G < T -- is the minimum of a key that holds
// the bases big-endian, 2 bits each (place_key_of_codes: integer order = string order): one 64-bit key for the first 32 bases, a second
// one for the bases 32 .. 61 among the records whose first key is the minimum.
//
// The same header is compiled by g++ for tests/emul/msa_place_emul.cpp (CPU test of the rule on 64 emulated lanes against
// functions.get_best_solution, also under -fsanitize=undefined,address).
#pragma once
#include "band_core.hpp"

namespace isocon {

static constexpr int PLACE_MAX_LONGEST = 62;          // longest insertion of a slot the device places: L = longest + 2 <= 64 lanes
static constexpr int PLACE_MAX_L = PLACE_MAX_LONGEST + 2;
static constexpr int PLACE_DP_STRIDE = PLACE_MAX_LONGEST;
static constexpr int PLACE_DP_BYTES = PLACE_MAX_L * PLACE_DP_STRIDE;          // rows 1 .. 64, columns 1 .. 62
static constexpr uint64_t PLACE_KEY_NONE = ~0ull;
enum { PLACE_SUBSTRING = 0, PLACE_THREADED = 1, PLACE_OFFSET = 2, PLACE_LEFT = 3 };          // which step placed a record

struct PlaceStr { uint64_t v, b0, b1; };

ISO_HD uint64_t place_low(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// mx of a representative (its bases in r0 / r1, bit j = base j): the bases move up one column behind the pad
ISO_HD PlaceStr place_padded(uint64_t r0, uint64_t r1, int longest)
{
    PlaceStr mx;
    mx.v = place_low(longest) << 1;
    mx.b0 = (r0 << 1) & mx.v;
    mx.b1 = (r1 << 1) & mx.v;
    return mx;
}

// bit t (t < m): q[t] == mx[p + t]; 0 <= p < 64
ISO_HD uint64_t place_eq(const PlaceStr &mx, const PlaceStr &q, int p)
{
    return ~((mx.b0 >> p) ^ q.b0) & ~((mx.b1 >> p) ^ q.b1) & (mx.v >> p) & q.v;
}

// q at offset p, gaps elsewhere
ISO_HD PlaceStr place_at(const PlaceStr &q, int p)
{
    PlaceStr o;
    o.v = q.v << p; o.b0 = q.b0 << p; o.b1 = q.b1 << p;
    return o;
}

// step 3's order of the offsets: the largest key wins -- most matches, then the smallest p; 0 = no match at p
ISO_HD uint32_t place_offset_key(const PlaceStr &mx, const PlaceStr &q, int p)
{
    const uint32_t n = (uint32_t)popc64(place_eq(mx, q, p));
    return n ? (n << 8) | (uint32_t)(255 - p) : 0u;
}
ISO_HD int place_offset_of_key(uint32_t key) { return key ? 255 - (int)(key & 255u) : 0; }

ISO_HD uint8_t place_char(const PlaceStr &o, int t)
{
    return (o.v >> t) & 1ull ? (uint8_t)("ACGT"[((o.b0 >> t) & 1ull) | (((o.b1 >> t) & 1ull) << 1)]) : (uint8_t)'-';
}

// DP cell (i, j), 1 <= i <= L, 1 <= j <= m, from its upper (i - 1, j), left (i, j - 1) and diagonal (i - 1, j - 1) neighbours
ISO_HD uint32_t place_dp_value(uint32_t up, uint32_t left, uint32_t diag, const PlaceStr &mx, const PlaceStr &q, int i, int j)
{
    const uint64_t same = ~((mx.b0 >> (i - 1)) ^ (q.b0 >> (j - 1))) & ~((mx.b1 >> (i - 1)) ^ (q.b1 >> (j - 1))) & (mx.v >> (i - 1)) & 1ull;
    uint32_t best = diag + (same ? 0u : 1u);
    if (up + 1u < best) best = up + 1u;
    if (left + 1u < best) best = left + 1u;
    return best;
}

ISO_HD int place_dp_index(int i, int j) { return (i - 1) * PLACE_DP_STRIDE + (j - 1); }
ISO_HD uint32_t place_dp_at(const uint8_t *D, int i, int j) { return i == 0 ? (uint32_t)j : j == 0 ? (uint32_t)i : (uint32_t)D[place_dp_index(i, j)]; }

#if defined(__HIP_DEVICE_COMPILE__)
#define PLACE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))          // (all lanes read the same cell: the walk stays on the scalar unit)
#else
#define PLACE_UNIFORM(x) (x)
#endif

// Step 2's backtrack over the stored cells: false if the walk takes a step in q alone; else o = the threaded columns.
ISO_HD bool place_thread(const uint8_t *D, int L, int m, const PlaceStr &q, PlaceStr &o)
{
    o.v = o.b0 = o.b1 = 0ull;
    int i = L, j = m;
    while (i > 0 || j > 0) {
        const uint32_t here = PLACE_UNIFORM(place_dp_at(D, i, j));
        if (i > 0 && PLACE_UNIFORM(place_dp_at(D, i - 1, j)) + 1u == here) { --i; continue; }          // mx alone: '-' in column i - 1
        if (j > 0 && PLACE_UNIFORM(place_dp_at(D, i, j - 1)) + 1u == here) return false;                // q alone
        --i; --j;
        o.v |= 1ull << i;
        o.b0 |= ((q.b0 >> j) & 1ull) << i;
        o.b1 |= ((q.b1 >> j) & 1ull) << i;
    }
    return true;
}

// ---- the representative's keys ---------------------------------------------------------------------------------------------------------

// the 2-bit groups of x in reverse order (group 0 <-> group 31)
ISO_HD uint64_t place_rev2(uint64_t x)
{
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
    x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
    return (x >> 32) | (x << 32);
}

// key of up to 32 bases given as a wide record gives them (base j at bits 2 j, zero behind the last): base 0 in the top two bits
ISO_HD uint64_t place_key_of_codes(uint64_t codes) { return place_rev2(codes); }

// key of the n <= 32 bases whose planes are p0 / p1 (base j at bit j)
ISO_HD uint64_t place_key_of_planes(uint64_t p0, uint64_t p1, int n)
{
    uint64_t key = 0;
    for (int j = 0; j < n; ++j) key |= (((p0 >> j) & 1ull) | (((p1 >> j) & 1ull) << 1)) << (62 - 2 * j);
    return key;
}

// code of base j (0 <= j < 64) of the string whose keys are k1 (bases 0 .. 31) and k2 (32 ..)
ISO_HD uint32_t place_key_code(uint64_t k1, uint64_t k2, int j) { return (uint32_t)(((j < 32 ? k1 : k2) >> (62 - 2 * (j & 31))) & 3ull); }

}  // namespace isocon
