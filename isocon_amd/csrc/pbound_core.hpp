// pbound_core.hpp -- lane-level math of Raghavan's bound of the statistical test (pbound.hpp), shared with the CPU emulator of tests/emul
// (g++, also under UBSan + ASan).  One test per lane; no cross-lane traffic, no LDS, no floating-point arithmetic.
//
// The reference (modules/hypothesis_test_module.py:253-329) evaluates, in 100-digit decimals, d = y / m - 1, k = m d and
// e^k / (1 + d)^(k + k / d), with y == 0 -> 1.0 and d == 0 -> 0.5, and converts the result to a double.  With 1 + d = y / m, k = y - m and
// k / d = m that number is
//         f(m, y) = exp(E),   E = (y - m) - y (ln y - ln m)  <= 0.
// pb_eval computes E and f in 320-bit fixed point (ten 32-bit limbs, 256 fraction bits; `ulp` below is 2^-256), carries a bound on the
// error of E through every step, and rounds f to a double only if the bits it discards are farther from the halfway pattern than
// that bound times 2^22 (PB_SLACK): then float() of the reference's decimal is the same double, because the reference's own
// deviation from f -- below 10^-89 relative inside the domain -- is one of the bound's terms.  Otherwise the test is
// `not certified` and the caller evaluates it with the reference statement.
//
//   ln x         x = M 2^(e - 52), M the 53-bit mantissa: ln x = (e + 1) ln 2 - A(M), A(M) = -ln(M / 2^53) in (0, ln 2].  M / 2^53 in [1/2, 1) is
//                multiplied up to x' in (1 - 2^-16, 1] by the factors (1 + 2^-k), k = 1 .. 16, each taken iff the product stays <= 1 (the
//                products are exact: 53 + 136 bits); A = sum of the taken ln(1 + 2^-k) + sum_{n = 1 .. 18} u^n / n, u = 1 - x' (Horner).
//   E            L = ln y - ln m = (e_y - e_m) ln 2 + A(M_m) - A(M_y); y L = M_y |L| shifted by y's exponent (y exact); y - m from the two
//                doubles written to fixed point (exact wherever 2^-256 resolves them: only the absolute error of E matters, as it is
//                the relative error of f, so the cancellation at y ~ m costs nothing).
//   exp          -E = n ln 2 - r, r in [0, ln 2]: r loses the ln(1 + 2^-k) it can (k = 1 .. 16), exp of the rest (< 2^-16) is
//                sum_{n = 0 .. 15} r^n / n! (Horner), the taken factors come back as g += g >> k; f = g 2^-n, g in [1, 2).
//   rounding     the double's ulp is 2^p ulp of g, p = 204 for a normal result and 204 + (n - 1022) in the subnormal range; g / 2^p is
//                rounded to nearest, certified iff | g mod 2^p - 2^(p - 1) | > err_total 2^22.  -E >= 800: f < 2^-1154, 0.0.
// Error terms, in ulp: every table entry < 1, a product (pb_mul) <= 8, so A <= 32 (PB_ERR_A), L <= |e_y - e_m| + 64, y L <=
// (floor(y) + 1) err(L) + 1, y - m <= 2, n ln 2 <= n, the exponential <= 159 and the reference's deviation <= 1 (PB_ERR_EXP = 160).
// Certified domain: m and y normal, positive, below 2^31; y |ln(y / m)| and |y - m| below PB_DOMAIN = floor(9 10^5 ln 10) (beyond,
// the reference's decimals leave their exponent range); and e_y - e_m >= -PB_MIN_DE, i.e. y / m > 2^-301: the reference forms 1 + d from
// d = y / m - 1 rounded to 100 digits, which keeps 100 - log10(m / y) digits of y / m and none below y / m = 5 10^-101, where it raises
// (0 ** 0).  y == 0 (-> 1.0) and y == m (-> 0.5) are decided on the doubles' bits.
#pragma once
#include "band_core.hpp"

namespace isocon {

enum : int { PB_F = 8, PB_NL = 10, PB_SLACK = 22, PB_MIN_DE = 300 };
enum : uint32_t { PB_ERR_A = 32u, PB_ERR_EXP = 160u, PB_DOMAIN = 2072326u, PB_ZERO_AT = 800u };

// floor(value 2^256), least significant limb first
static constexpr uint32_t PB_LN2[8] = {0x8baafa2bu, 0x8a0d175bu, 0x7298b62du, 0x40f34326u, 0x03f2f6afu, 0xc9e3b398u, 0xd1cf79abu, 0xb17217f7u};
static constexpr uint32_t PB_LN1P[16][8] = {
    {0xc59e3b60u, 0xb38ad78eu, 0x4547d7c2u, 0x7d20ffb3u, 0x01488606u, 0xda35d9bdu, 0xfe612fcau, 0x67cc8fb2u},          // ln(1 + 2^-1)
    {0x64bfc746u, 0x70f133f5u, 0x11adc1b1u, 0xc765ea74u, 0xff734495u, 0x4bb03de5u, 0x35344358u, 0x391fef8fu},          // ln(1 + 2^-2)
    {0xff917c95u, 0xdd0897c1u, 0x17f6f957u, 0xb94ebc40u, 0xfe9e155du, 0xea87ffe1u, 0x2af2e5e9u, 0x1e27076eu},          // ln(1 + 2^-3)
    {0x96f69849u, 0x71851f0au, 0x75b52596u, 0xd3474d33u, 0x75997898u, 0xbe64b8b7u, 0x08b15330u, 0x0f851860u},          // ln(1 + 2^-4)
    {0xe3673dcdu, 0xdf6c758fu, 0xddf35ad1u, 0xaefae14cu, 0xef229faeu, 0x3e3f04f1u, 0x9e0cc013u, 0x07e0a6c3u},          // ln(1 + 2^-5)
    {0x77122f83u, 0xd140fe05u, 0x3ddc5335u, 0xeb03be90u, 0x6f57aadbu, 0xf3db4e9au, 0x1f807c79u, 0x03f81516u},          // ln(1 + 2^-6)
    {0x6b5788c3u, 0x76702788u, 0xf9a073a8u, 0xb3db2c3eu, 0x1dc282d2u, 0xc3769039u, 0xb106788fu, 0x01fe02a6u},          // ln(1 + 2^-7)
    {0x5a1a3322u, 0x91ba6e33u, 0x6d725824u, 0x8ccd29ddu, 0xda6a5bb4u, 0x50435ab4u, 0x15885e02u, 0x00ff8055u},          // ln(1 + 2^-8)
    {0x12ace6e8u, 0xc73356ccu, 0xe89a011eu, 0xcad8ec22u, 0x3e3b1ab1u, 0xe29e3a15u, 0xa6ac4399u, 0x007fe00au},          // ln(1 + 2^-9)
    {0xa6eb720cu, 0x6e34c564u, 0x62ef4eb0u, 0x8e30d617u, 0x2499268eu, 0x7809a0a3u, 0x5515621fu, 0x003ff801u},          // ln(1 + 2^-10)
    {0x5c09d7acu, 0x4e588a36u, 0xe5e0fc9eu, 0x545eb8e9u, 0xb318cb38u, 0x06678ad8u, 0x2aa6ab11u, 0x001ffe00u},          // ln(1 + 2^-11)
    {0x8222f25fu, 0xc9b2e919u, 0x8002d083u, 0x49c8cd0bu, 0xe271ee05u, 0x885de026u, 0x05551558u, 0x000fff80u},          // ln(1 + 2^-12)
    {0xc4b26860u, 0x46c08a95u, 0xde4647beu, 0x6a90d794u, 0x2bc2bf0fu, 0xc443999eu, 0x00aaa6aau, 0x0007ffe0u},          // ln(1 + 2^-13)
    {0x3228bbdau, 0xf7b8170bu, 0x08a27c47u, 0x0dcf437au, 0x809be9c1u, 0x56221f77u, 0x00155515u, 0x0003fff8u},          // ln(1 + 2^-14)
    {0x8c5ae43bu, 0x582a09b1u, 0x82c24db8u, 0xf8e86e20u, 0x6678af6au, 0xaab11106u, 0x0002aaa6u, 0x0001fffeu},          // ln(1 + 2^-15)
    {0x1876afc0u, 0xaf1e4b66u, 0xaff31675u, 0x07028c98u, 0x5dde0270u, 0x15558888u, 0x80005555u, 0x0000ffffu},          // ln(1 + 2^-16)
};
static constexpr uint32_t PB_INV[17][8] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u},          // 1 / 2
    {0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u},          // 1 / 3
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u},          // 1 / 4
    {0x33333333u, 0x33333333u, 0x33333333u, 0x33333333u, 0x33333333u, 0x33333333u, 0x33333333u, 0x33333333u},          // 1 / 5
    {0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0x2aaaaaaau},          // 1 / 6
    {0x92492492u, 0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u},          // 1 / 7
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x20000000u},          // 1 / 8
    {0x71c71c71u, 0x1c71c71cu, 0xc71c71c7u, 0x71c71c71u, 0x1c71c71cu, 0xc71c71c7u, 0x71c71c71u, 0x1c71c71cu},          // 1 / 9
    {0x99999999u, 0x99999999u, 0x99999999u, 0x99999999u, 0x99999999u, 0x99999999u, 0x99999999u, 0x19999999u},          // 1 / 10
    {0x745d1745u, 0x5d1745d1u, 0x1745d174u, 0x45d1745du, 0xd1745d17u, 0x745d1745u, 0x5d1745d1u, 0x1745d174u},          // 1 / 11
    {0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x55555555u, 0x15555555u},          // 1 / 12
    {0xb13b13b1u, 0x13b13b13u, 0x3b13b13bu, 0xb13b13b1u, 0x13b13b13u, 0x3b13b13bu, 0xb13b13b1u, 0x13b13b13u},          // 1 / 13
    {0x49249249u, 0x92492492u, 0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u, 0x49249249u, 0x12492492u},          // 1 / 14
    {0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u},          // 1 / 15
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x10000000u},          // 1 / 16
    {0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu, 0x0f0f0f0fu},          // 1 / 17
    {0x38e38e38u, 0x8e38e38eu, 0xe38e38e3u, 0x38e38e38u, 0x8e38e38eu, 0xe38e38e3u, 0x38e38e38u, 0x0e38e38eu},          // 1 / 18
};
static constexpr uint32_t PB_INVFACT[14][8] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u},          // 1 / 2!
    {0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0x2aaaaaaau},          // 1 / 3!
    {0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0xaaaaaaaau, 0x0aaaaaaau},          // 1 / 4!
    {0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u, 0x22222222u, 0x02222222u},          // 1 / 5!
    {0x5b05b05bu, 0xb05b05b0u, 0x05b05b05u, 0x5b05b05bu, 0xb05b05b0u, 0x05b05b05u, 0x5b05b05bu, 0x005b05b0u},          // 1 / 6!
    {0x0d00d00du, 0xd00d00d0u, 0x00d00d00u, 0x0d00d00du, 0xd00d00d0u, 0x00d00d00u, 0x0d00d00du, 0x000d00d0u},          // 1 / 7!
    {0x01a01a01u, 0x1a01a01au, 0xa01a01a0u, 0x01a01a01u, 0x1a01a01au, 0xa01a01a0u, 0x01a01a01u, 0x0001a01au},          // 1 / 8!
    {0x002e3bc7u, 0x583911cau, 0xd8e671f5u, 0xe3bc74aau, 0x911ca002u, 0x671f5583u, 0xc74aad8eu, 0x00002e3bu},          // 1 / 9!
    {0x3337d2c7u, 0x559f4e94u, 0x7c170b65u, 0xe392d877u, 0x5b4fa999u, 0xd71cbbc0u, 0x93edde27u, 0x0000049fu},          // 1 / 10!
    {0x04a7fbe3u, 0xaab1643cu, 0xdcbc46dau, 0x71c7880au, 0x1f92e0dfu, 0x138e3f9du, 0x99159fd5u, 0x0000006bu},          // 1 / 11!
    {0x55b8aa52u, 0xe38ec85au, 0xe7ba5b3cu, 0xf425f600u, 0x6d4c3d67u, 0x6c4bdaa2u, 0xf76c77fcu, 0x00000008u},          // 1 / 12!
    {0x06980d1au, 0x38e39942u, 0x9babdfa2u, 0xd7b4269du, 0x1c198e91u, 0x43684be5u, 0xb092309du, 0x00000000u},          // 1 / 13!
    {0xb75400efu, 0xbaebaf84u, 0x668c46d4u, 0xfd1f2754u, 0x5d6f8a2eu, 0x603e4e90u, 0x0c9cba54u, 0x00000000u},          // 1 / 14!
    {0x0c38ccdcu, 0x83ed943cu, 0x8f5eaf63u, 0x774657f4u, 0x8ec32b58u, 0x399dc0f8u, 0x00d73f9fu, 0x00000000u},          // 1 / 15!
};

template <int N> struct PbW { uint32_t w[N]; };
typedef PbW<PB_NL> PbFx;          // w[8], w[9]: the integer part

struct PbDiag { uint64_t err_total; int p; PbFx dist; };          // what the emulator reports: the error bound (ulp) and | g mod 2^p - 2^(p - 1) |

template <int N> ISO_HD PbW<N> pb_zero()
{
    PbW<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.w[i] = 0u;
    return r;
}

ISO_HD PbFx pb_frac(const uint32_t (&c)[8])
{
    PbFx r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = c[i];
    r.w[8] = r.w[9] = 0u;
    return r;
}

template <int N> ISO_HD PbW<N> pb_select(bool c, const PbW<N> &a, const PbW<N> &b)
{
    PbW<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) r.w[i] = c ? a.w[i] : b.w[i];
    return r;
}

// a + b (mod 2^(32 N)); *carry: the bit that left
template <int N> ISO_HD PbW<N> pb_add(const PbW<N> &a, const PbW<N> &b, uint32_t *carry = nullptr)
{
    PbW<N> r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        c += (uint64_t)a.w[i] + b.w[i];
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    if (carry) *carry = (uint32_t)c;
    return r;
}

// a - b (mod 2^(32 N)); *borrow: 1 iff a < b
template <int N> ISO_HD PbW<N> pb_sub(const PbW<N> &a, const PbW<N> &b, uint32_t *borrow = nullptr)
{
    PbW<N> r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t d = (uint64_t)a.w[i] - b.w[i] - c;
        r.w[i] = (uint32_t)d;
        c = (d >> 32) & 1u;
    }
    if (borrow) *borrow = (uint32_t)c;
    return r;
}

template <int N> ISO_HD bool pb_less(const PbW<N> &a, const PbW<N> &b)
{
    uint32_t borrow;
    (void)pb_sub(a, b, &borrow);
    return borrow != 0u;
}

// a >> s, any s (the bits that leave are dropped: < 1 ulp)
template <int N> ISO_HD PbW<N> pb_shr(PbW<N> a, uint32_t s)
{
    const uint32_t q = s >> 5, b = s & 31u;
#pragma unroll
    for (int st = 1; st < N; st <<= 1) {
        const bool on = (q & (uint32_t)st) != 0u;
        PbW<N> t;
#pragma unroll
        for (int i = 0; i < N; ++i) t.w[i] = on ? (i + st < N ? a.w[i + st] : 0u) : a.w[i];
        a = t;
    }
    PbW<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t two = (uint64_t)(i + 1 < N ? a.w[i + 1] : 0u) << 32 | a.w[i];
        r.w[i] = s >= 32u * N ? 0u : (uint32_t)(two >> b);
    }
    return r;
}

// a << s (mod 2^(32 N)), any s
template <int N> ISO_HD PbW<N> pb_shl(PbW<N> a, uint32_t s)
{
    const uint32_t q = s >> 5, b = s & 31u;
#pragma unroll
    for (int st = 1; st < N; st <<= 1) {
        const bool on = (q & (uint32_t)st) != 0u;
        PbW<N> t;
#pragma unroll
        for (int i = 0; i < N; ++i) t.w[i] = on ? (i - st >= 0 ? a.w[i - st] : 0u) : a.w[i];
        a = t;
    }
    PbW<N> r;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint64_t two = (uint64_t)a.w[i] << 32 | (i > 0 ? a.w[i - 1] : 0u);
        r.w[i] = s >= 32u * N ? 0u : (uint32_t)((two << b) >> 32);
    }
    return r;
}

// a b, both < 2^32 in value and the product too: the columns below the guard limb are dropped, <= 8 ulp too small
ISO_HD PbFx pb_mul(const PbFx &a, const PbFx &b)
{
    PbFx r;
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int c = PB_F - 1; c < PB_F + PB_NL; ++c) {
#pragma unroll
        for (int i = 0; i < PB_NL; ++i) {
            const int j = c - i;
            if (j >= 0 && j < PB_NL) {
                const uint64_t p = (uint64_t)a.w[i] * b.w[j];
                lo += (uint32_t)p;
                hi += p >> 32;
            }
        }
        if (c >= PB_F) r.w[c - PB_F] = (uint32_t)lo;
        lo = (lo >> 32) + hi;
        hi = 0;
    }
    return r;
}

// a k, exact (the caller knows that it fits)
ISO_HD PbFx pb_mul_small(const PbFx &a, uint32_t k)
{
    PbFx r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < PB_NL; ++i) {
        c += (uint64_t)a.w[i] * k;
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}

// a M, exact, twelve limbs
ISO_HD PbW<PB_NL + 2> pb_mul_u64(const PbFx &a, uint64_t M)
{
    PbW<PB_NL + 2> r;
    const uint32_t m0 = (uint32_t)M, m1 = (uint32_t)(M >> 32);
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < PB_NL + 2; ++c) {
        if (c < PB_NL) { const uint64_t p = (uint64_t)a.w[c] * m0; lo += (uint32_t)p; hi += p >> 32; }
        if (c >= 1 && c - 1 < PB_NL) { const uint64_t p = (uint64_t)a.w[c - 1] * m1; lo += (uint32_t)p; hi += p >> 32; }
        r.w[c] = (uint32_t)lo;
        lo = (lo >> 32) + hi;
        hi = 0;
    }
    return r;
}

ISO_HD PbFx pb_one()
{
    PbFx r = pb_zero<PB_NL>();
    r.w[8] = 1u;
    return r;
}

// A(M) = -ln(M / 2^53) for a 53-bit mantissa M (bit 52 set), <= PB_ERR_A ulp off
ISO_HD PbFx pb_neg_ln_mantissa(uint64_t M)
{
    PbFx x = pb_zero<PB_NL>(), sum = pb_zero<PB_NL>();
    x.w[6] = (uint32_t)(M << 11);
    x.w[7] = (uint32_t)((M << 11) >> 32);
    for (int k = 1; k <= 16; ++k) {
        const PbFx t = pb_add(x, pb_shr(x, (uint32_t)k));
        uint32_t low = 0u;
#pragma unroll
        for (int i = 0; i < PB_F; ++i) low |= t.w[i];
        const bool take = t.w[9] == 0u && (t.w[8] == 0u || (t.w[8] == 1u && low == 0u));          // x (1 + 2^-k) <= 1
        x = pb_select(take, t, x);
        sum = pb_select(take, pb_add(sum, pb_frac(PB_LN1P[k - 1])), sum);
    }
    const PbFx u = pb_sub(pb_one(), x);
    PbFx p = pb_frac(PB_INV[16]);
    for (int n = 17; n >= 2; --n) p = pb_add(pb_frac(PB_INV[n - 2]), pb_mul(u, p));
    p = pb_add(pb_one(), pb_mul(u, p));
    return pb_add(sum, pb_mul(u, p));
}

// a positive normal double below 2^64 as fixed point (bits below 2^-256 dropped); e: its unbiased exponent, M: its mantissa
ISO_HD PbFx pb_from_double(uint64_t M, int e)
{
    PbFx v = pb_zero<PB_NL>();
    v.w[8] = (uint32_t)(M << 11);
    v.w[9] = (uint32_t)((M << 11) >> 32);          // M 2^11 = x 2^(63 - e)
    return pb_shr(v, (uint32_t)(63 - e));
}

// The bound of one test from the bits of m_sum and y_sum: the bits of the double; *certified as the header says (0: the bits are 0).
ISO_HD uint64_t pb_eval(uint64_t m_bits, uint64_t y_bits, uint8_t *certified, PbDiag *diag = nullptr)
{
    const uint32_t fm = (uint32_t)(m_bits >> 52), fy = (uint32_t)(y_bits >> 52);          // sign and exponent field
    const bool m_ok = fm >= 1u && fm <= 1023u + 30u;          // positive, normal, < 2^31
    const bool y_ok = fy >= 1u && fy <= 1023u + 30u;
    const uint64_t Mm = (m_bits & 0xfffffffffffffull) | 1ull << 52, My = (y_bits & 0xfffffffffffffull) | 1ull << 52;
    const int em = (int)(fm & 2047u) - 1023, ey = (int)(fy & 2047u) - 1023;
    const bool up = y_bits > m_bits;          // y > m (positive doubles order as their bits)
    // L = ln y - ln m and its error
    const int de = ey - em;
    const uint32_t ade = (uint32_t)(de < 0 ? -de : de);
    const PbFx steps = pb_mul_small(pb_frac(PB_LN2), ade & 4095u);
    const PbFx plus = pb_add(pb_neg_ln_mantissa(Mm), de > 0 ? steps : pb_zero<PB_NL>());
    const PbFx minus = pb_add(pb_neg_ln_mantissa(My), de < 0 ? steps : pb_zero<PB_NL>());
    uint32_t wrong_l;
    const PbFx L = pb_sub(pb_select(up, plus, minus), pb_select(up, minus, plus), &wrong_l);          // |L|, its sign is that of y - m
    const uint64_t err_l = (uint64_t)ade + 2u * PB_ERR_A;
    // y |L|, y exact; |y - m|
    const PbW<PB_NL + 2> wide = pb_shr(pb_mul_u64(L, My), (uint32_t)(52 - ey));
    PbFx P;
#pragma unroll
    for (int i = 0; i < PB_NL; ++i) P.w[i] = wide.w[i];
    const PbFx fx_m = pb_from_double(Mm, em), fx_y = pb_from_double(My, ey);
    const PbFx D = pb_sub(pb_select(up, fx_y, fx_m), pb_select(up, fx_m, fx_y));
    const uint64_t y_floor = (uint64_t)fx_y.w[9] << 32 | fx_y.w[8];
    const uint64_t err_z = (y_floor + 1u) * err_l + 3u;
    const bool in_domain = m_ok && y_ok && de >= -PB_MIN_DE && wrong_l == 0u && wide.w[10] == 0u && wide.w[11] == 0u && P.w[9] == 0u && P.w[8] < PB_DOMAIN && D.w[9] == 0u &&
                           D.w[8] < PB_DOMAIN;
    // Z = -E = y L - (y - m) >= 0 (below 0 by less than the error: 0)
    uint32_t below;
    PbFx Z = pb_sub(pb_select(up, P, D), pb_select(up, D, P), &below);
    Z = pb_select(below != 0u, pb_zero<PB_NL>(), Z);
    const bool is_zero = Z.w[9] != 0u || Z.w[8] >= PB_ZERO_AT;
    // Z = n ln 2 - r
    const PbFx ln2 = pb_frac(PB_LN2);
    const uint64_t z_top = (uint64_t)(Z.w[8] & 1023u) << 32 | Z.w[7];
    uint32_t n = (uint32_t)((z_top * 1512775ull) >> 52) + 1u;          // floor(2^20 / ln 2): n - 1 is floor(Z / ln 2) or one less
    PbFx t = pb_mul_small(ln2, n);
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool low = pb_less(t, Z);
        t = pb_select(low, pb_add(t, ln2), t);
        n += low ? 1u : 0u;
    }
    PbFx r = pb_sub(t, Z);
#pragma unroll
    for (int fix = 0; fix < 2; ++fix) {
        const bool high = !pb_less(r, ln2) && n > 0u;
        r = pb_select(high, pb_sub(r, ln2), r);
        n -= high ? 1u : 0u;
    }
    // g = exp(r)
    uint32_t taken = 0u;
    for (int k = 1; k <= 16; ++k) {
        const PbFx c = pb_frac(PB_LN1P[k - 1]);
        const bool take = !pb_less(r, c);
        r = pb_select(take, pb_sub(r, c), r);
        taken |= take ? 1u << k : 0u;
    }
    PbFx g = pb_frac(PB_INVFACT[13]);
    for (int i = 14; i >= 2; --i) g = pb_add(pb_frac(PB_INVFACT[i - 2]), pb_mul(r, g));
    g = pb_add(pb_one(), pb_mul(r, g));
    g = pb_add(pb_one(), pb_mul(r, g));
    for (int k = 1; k <= 16; ++k) g = pb_select((taken >> k & 1u) != 0u, pb_add(g, pb_shr(g, (uint32_t)k)), g);
    const bool two = g.w[8] >= 2u;
    g = pb_select(two, pb_shr(g, 1u), g);
    n -= two && n > 0u ? 1u : 0u;
    const uint64_t err_total = err_z + n + PB_ERR_EXP;
    // round g 2^-n to a double
    const uint32_t p = 204u + (n > 1022u ? n - 1022u : 0u);
    const bool tiny = p >= 259u;          // g 2^-p < 1 / 4
    const PbFx kept = pb_shr(g, p);
    const PbFx rest = pb_shl(g, 320u - (tiny ? 258u : p));          // (g mod 2^p) 2^(320 - p)
    const bool round_up = (rest.w[9] >> 31) != 0u;
    PbFx half = pb_zero<PB_NL>();
    half.w[9] = 0x80000000u;
    PbFx dist = pb_shr(pb_sub(pb_select(round_up, rest, half), pb_select(round_up, half, rest)), 320u - (tiny ? 258u : p));
    PbFx margin = pb_zero<PB_NL>();
    margin.w[0] = (uint32_t)err_total;
    margin.w[1] = (uint32_t)(err_total >> 32);
    margin = pb_shl(margin, (uint32_t)PB_SLACK);
    const bool err_small = err_total < 1ull << 60;
    const bool clear = err_small && (is_zero || tiny || pb_less(margin, dist));
    const uint64_t mant = ((uint64_t)kept.w[1] << 32 | kept.w[0]) + (round_up ? 1u : 0u);
    uint64_t bits = ((uint64_t)(n < 1022u ? 1022u - n : 0u) << 52) + mant;
    if (is_zero || tiny) bits = 0ull;
    bool ok = in_domain && clear;
    // the special cases come first (m must still be a number the reference divides by)
    if (m_ok && y_bits == 0ull) { bits = 0x3ff0000000000000ull; ok = true; }
    else if (m_ok && y_bits == m_bits) { bits = 0x3fe0000000000000ull; ok = true; }
    if (diag) { diag->err_total = err_total; diag->p = (int)p; diag->dist = dist; }
    *certified = ok ? 1u : 0u;
    return ok ? bits : 0ull;
}

}  // namespace isocon
