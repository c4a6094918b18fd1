// nn_surv_core.hpp -- which pairs of one batch of the survivor-list builder (nn_list.hpp, k_nn_survivors) are kept, where they go in the
// staging buffer, and when a chunk leaves it.  Shared by the kernel and its CPU emulators (tests/emul/survivor_groups_emul.cpp,
// tests/emul/surv_packed_emul.cpp).
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

// ---- which pairs of a batch are kept: the test of one pair, and of a lane's four pairs at once ------------------------------------------
// x is the entry of the wave, y the partner at one row position; side 0 = x's own row (y above x), side 1 = its transposed row.
//   inr                the position is inside the row
//   x_isq, x_ist, y_isq, y_ist    roles: queries / is a target.  x queries y iff x_isq and y_ist; y queries x iff y_isq and x_ist
//   kx0, thr_y         thresholds min(best, length, 64) of x and y; kcap: the cap of the pass
//   m, len_y           lengths;  bound: the pair's q-gram bound;  sx, sy: hub scores (9 bits)
//   class_mode         0 = class per pair, -1 = every pair in the 64-row class, +1 = pairs above the 32-row form's threshold leave (nn_list.hpp)
// A pair is a CANDIDATE if it has a direction and its length difference is within the threshold k = min(max over its directions, kcap),
// ACCEPTED if its bound is too, MINE if x owns it (larger hub score, ties to the lower index: side 0 is the lower end).
struct SurvTest { bool cand, accept, mine, wide, keep, to_narrow; };
static constexpr int32_t SURV_NARROW_K = 31;          // (= NN_NARROW_K: thresholds of the 32-row class)

ISO_HD SurvTest surv_test(bool inr, bool x_isq, bool x_ist, bool y_isq, bool y_ist, int32_t kx0, int32_t thr_y, int32_t kcap, int32_t m, int32_t len_y, uint32_t bound,
                          uint32_t sx, uint32_t sy, int side, int32_t class_mode)
{
    SurvTest t;
    const bool xq = inr && x_isq && y_ist;        // x queries y
    const bool yq = inr && x_ist && y_isq;        // y queries x
    int32_t kx = -1, ky = -1;
    if (xq) kx = kx0;
    if (yq) ky = thr_y;
    int32_t k = kx > ky ? kx : ky;
    if (k > kcap) k = kcap;
    const int32_t dl = m - len_y, ad = dl < 0 ? -dl : dl;
    t.cand = inr && k >= 0 && ad <= k;
    t.accept = t.cand && (int32_t)bound <= k;
    t.mine = t.accept && (side == 0 ? sy <= sx : sx > sy);
    t.wide = t.mine && class_mode > 0 && k > SURV_NARROW_K;
    t.keep = t.mine && !t.wide;
    t.to_narrow = t.keep && class_mode >= 0 && k <= SURV_NARROW_K;
    return t;
}

// The same test on the four positions of a lane at once, a byte per position (class_mode <= 0).  With
//   a = (x queries y) ? min(kx0, kcap) + 1 : 0    and    b = (y queries x) ? min(thr_y, kcap) + 1 : 0        (both in 0 .. 64 for kcap <= 63)
// k + 1 = max(a, b), "no direction" is 0, and   accept = (ad < a or ad < b) and (bound < a or bound < b),   to_narrow = a <= 32 and b <= 32.
// v < c for bytes v < 128, c <= 128: (v | 0x80) - c has bit 7 clear, and no byte borrows from its neighbour.  What needs the partner
// comes from three arrays with one item per entry, written once per pass (k_nn_entry_meta) with the guard bits in place:
//   role byte    is target << 7 | (is query ? min(thr, kcap) + 1 : 0)
//   length byte  0x80 | length & 127: inside a row 0 <= ad <= 63 (rows end where the lengths differ by more than 63 and lengths ascend),
//                so ad is the difference of the lengths modulo 128
//   score half   0x8000 | score
// and what is x's is the same in every byte (SurvX, wave-uniform).  REQUIRES kcap <= 63, a length-sorted store, class_mode <= 0.
static constexpr uint32_t SURV_H = 0x80808080u;
ISO_HD uint8_t surv_role_byte(bool is_t, bool is_q, int32_t thr, int32_t kcap)
{
    const int32_t c = kcap < 63 ? (kcap < 0 ? 0 : kcap) : 63, k = thr < c ? thr : c;
    return (uint8_t)((is_t ? 0x80u : 0u) | (is_q ? (uint32_t)(k < 0 ? 0 : k) + 1u : 0u));
}
ISO_HD uint8_t surv_len_byte(uint32_t len) { return (uint8_t)(0x80u | (len & 0x7fu)); }
ISO_HD uint16_t surv_score_half(uint32_t score) { return (uint16_t)(0x8000u | (score & 0x1ffu)); }

struct SurvX {
    uint32_t a4;          // a of the pairs whose partner is a target, in every byte (0: x does not query)
    uint32_t bm;          // the bits of a role byte that are b: 0x7f in every byte if x is a target, else 0
    uint32_t m4;          // side 0: m & 127 in every byte; side 1: (m & 127) + 1
    uint32_t s2;          // the score a partner has to stay below for x to own the pair, in both halves: sx + 1 on side 0, sx on side 1
    uint32_t nb;          // 33 in every byte if x is a target (b <= 32), else 0x80 (b = 0)
    uint32_t ua;          // bit 7 of every byte if a > 32 for a partner that is a target
    uint32_t cm;          // bit 7 of every byte if pairs have a class of their own (class_mode 0)
};
ISO_HD SurvX surv_x(bool x_isq, bool x_ist, int32_t kx0, int32_t kcap, int32_t m, uint32_t sx, int side, int32_t class_mode)
{
    SurvX X;
    const uint32_t a = x_isq ? (uint32_t)(kx0 < kcap ? kx0 : kcap) + 1u : 0u;
    X.a4 = a * 0x01010101u;
    X.bm = x_ist ? 0x7f7f7f7fu : 0u;
    X.m4 = (((uint32_t)m & 0x7fu) + (side == 0 ? 0u : 1u)) * 0x01010101u;
    X.s2 = (sx + (side == 0 ? 1u : 0u)) * 0x00010001u;
    X.nb = x_ist ? 0x21212121u : SURV_H;
    X.ua = a > (uint32_t)SURV_NARROW_K + 1u ? SURV_H : 0u;
    X.cm = class_mode >= 0 ? SURV_H : 0u;
    return X;
}

// the bytes of the positions inside the row, for a lane that has n of its four there (n <= 0: none, n >= 4: all)
ISO_HD uint32_t surv_inr_bytes(int32_t n) { return n <= 0 ? 0u : n >= 4 ? ~0u : (1u << (8 * n)) - 1u; }

// bytes 1 and 3 of lo, then of hi (bits 15 and 31 of two dwords to bit 7 of four bytes)
ISO_HD uint32_t surv_odd_bytes(uint32_t lo, uint32_t hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x07050301u);
#else
    return ((lo >> 8) & 0xffu) | ((lo >> 16) & 0xff00u) | ((hi << 8) & 0xff0000u) | (hi & 0xff000000u);
#endif
}

// bound: the four bounds; role: the role bytes, those of positions outside the row cleared (surv_inr_bytes); len7: the length bytes;
// s01, s23: the score halves.  Bit 7 of byte b of cand / accept / keep = the test of position b (keep: accepted and x's own).
template <int SIDE>
ISO_HD void surv_test4(const SurvX &X, uint32_t bound, uint32_t role, uint32_t len7, uint32_t s01, uint32_t s23, uint32_t &cand, uint32_t &accept, uint32_t &keep)
{
    const uint32_t d0 = len7 - X.m4;                                   // side 0: 128 + l - m per byte; side 1: 127 + l - m = 127 - (m - l)
    const uint32_t d = (SIDE == 0 ? d0 : ~d0) | SURV_H;                // 0x80 | ad
    const uint32_t b4 = role & X.bm;
    const uint32_t e = bound | SURV_H;
    const uint32_t c1 = (~(d - X.a4) & role) | ~(d - b4);              // bit 7: ad < a (partner is a target) or ad < b
    const uint32_t c2 = (~(e - X.a4) & role) | ~(e - b4);              // the same for the bound's low seven bits
    cand = c1 & SURV_H;
    accept = cand & c2 & ~bound;                                       // (a bound of 128 or more is above every threshold)
    keep = accept & ~surv_odd_bytes(s01 - X.s2, s23 - X.s2);           // bits 15, 31 of a difference: clear iff the partner's score is below s2
}
// bit 7 of byte b: a kept pair at position b belongs to the 32-row class
ISO_HD uint32_t surv_narrow4(const SurvX &X, uint32_t role) { return ~(((role | SURV_H) - X.nb) | (role & X.ua)) & X.cm; }

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
