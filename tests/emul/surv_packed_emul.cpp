// The keep test of the survivor-list builder on a lane's four pairs at once (isocon_amd/csrc/nn_surv_core.hpp surv_test4, surv_narrow4)
// against the test of one pair (surv_test, the definition).  A program of its own for tests/test_surv_packed_core.py (g++, plain and with
// -fsanitize=address,undefined; "quick" as the first argument thins the exhaustive sweep for the sanitized build).
//   1. sweep: bound 0 .. 255 x ad 0 .. 127 x a 0 .. 65 x b 0 .. 65, every tuple once (1.4 10^8 single tests).  The four bytes of a word hold
//      four tuples of the sweep under one a and rotate with a, so every (bound, ad, b) and every a is tested in each of the four byte
//      positions; everything else is random per word: side, the partner's target flag, x's target flag,
//      positions inside the row (0 .. 4), class mode -1 / 0 / +1, scores (equal, 0 and 511 among them).  The cap of the sweep is 64 so
//      that a and b reach 65; the role bytes are written directly.
//   2. caps: kcap 0, 31, 63 through surv_role_byte and surv_x (the cap folded into the role byte), thresholds 0 .. 64, every combination
//      of the four roles (no direction among them), every count of positions inside the row, both sides, the three class modes.
//   3. rows: the scan of a whole row as k_nn_survivors runs it -- four batches per iteration, an iteration without a kept pair skipped,
//      ballots from the byte masks -- against the scan with one test per pair, both through surv_batch into a staging buffer of
//      chunk + 64 words: the same writes, the same chunks at the same places, the same remainder, the same counts; on the row lengths
//      and chunk sizes of tests/emul/survivor_groups_emul.cpp.
// Class mode +1 has no packed form in the kernel; its outputs follow from the masks (wide = keep and not narrow, keep = to_narrow = keep
// and narrow), and that relation is what the sweep checks for it.
// stdout: "ok <sweep tuples> <cap cases> <rows> <chunks> <kept pairs>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../isocon_amd/csrc/nn_surv_core.hpp"

using namespace isocon;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static inline uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static uint32_t pick_score(uint32_t r, uint32_t sx)
{
    switch (r % 6) {
    case 0: return sx;
    case 1: return 0;
    case 2: return 511;
    case 3: return sx ? sx - 1 : 0;
    case 4: return sx < 511 ? sx + 1 : 511;
    default: return (r >> 8) % 512;
    }
}

struct Partner {
    bool ist, isq;
    int32_t thr, len;
    uint32_t bound, score;
    uint8_t role;          // as the packed test reads it
};

static unsigned long long n_fail = 0;

// one word of four partners against the four single tests
static bool check_word(bool x_isq, bool x_ist, int32_t kx0, int32_t kcap, int32_t m, uint32_t sx, int side, int32_t class_mode, int n_in, const Partner (&y)[4])
{
    const SurvX X = surv_x(x_isq, x_ist, kx0, kcap, m, sx, side, class_mode);
    uint32_t bound = 0, role = 0, len7 = 0, s01 = 0, s23 = 0;
    for (int p = 0; p < 4; ++p) {
        bound |= y[p].bound << (8 * p);
        role |= (uint32_t)y[p].role << (8 * p);
        len7 |= (uint32_t)surv_len_byte((uint32_t)y[p].len) << (8 * p);
        (p < 2 ? s01 : s23) |= (uint32_t)surv_score_half(y[p].score) << (16 * (p & 1));
    }
    role &= surv_inr_bytes(n_in);
    uint32_t cand, accept, keep;
    if (side == 0) surv_test4<0>(X, bound, role, len7, s01, s23, cand, accept, keep);
    else surv_test4<1>(X, bound, role, len7, s01, s23, cand, accept, keep);
    const uint32_t narrow = keep & surv_narrow4(X, role);
    bool ok = ((cand | accept | keep | narrow) & ~SURV_H) == 0;
    for (int p = 0; p < 4; ++p) {
        const SurvTest t = surv_test(p < n_in, x_isq, x_ist, y[p].isq, y[p].ist, kx0, y[p].thr, kcap, m, y[p].len, y[p].bound, sx, y[p].score, side, class_mode);
        const bool c = (cand >> (8 * p + 7)) & 1, a = (accept >> (8 * p + 7)) & 1, k = (keep >> (8 * p + 7)) & 1, nr = (narrow >> (8 * p + 7)) & 1;
        bool same = c == t.cand && a == t.accept && k == t.mine;
        if (class_mode > 0) same = same && t.wide == (k && !nr) && t.keep == nr && t.to_narrow == nr;
        else same = same && !t.wide && t.keep == k && t.to_narrow == nr;
        if (!same && n_fail++ < 10)
            fprintf(stderr, "mismatch: byte %d side %d mode %d inside %d xq %d xt %d kx0 %d kcap %d m %d sx %u | yt %d yq %d thr %d len %d bound %u score %u role %02x | packed %d%d%d%d single %d%d%d%d%d%d\n", p, side,
                    class_mode, n_in, (int)x_isq, (int)x_ist, kx0, kcap, m, sx, (int)y[p].ist, (int)y[p].isq, y[p].thr, y[p].len, y[p].bound, y[p].score, y[p].role, (int)c, (int)a, (int)k, (int)nr,
                    (int)t.cand, (int)t.accept, (int)t.mine, (int)t.wide, (int)t.keep, (int)t.to_narrow);
        ok = ok && same;
    }
    return ok;
}

static unsigned long long sweep(uint32_t bound_step)
{
    // tuple t = (bound, ad, b) under one a; byte p of word j holds tuple 4 j + (p + a) mod 4: every tuple is tested once under every a, and
    // over the values of a it sits in each of the four bytes, next to three other tuples of the sweep
    const uint32_t nb = (255u / bound_step) + 1u, N = nb * 128u * 66u;
    unsigned long long words = 0;
    for (int a = 0; a <= 65; ++a) {
        const bool x_isq = a > 0;
        const int32_t kx0 = x_isq ? a - 1 : (int32_t)(rnd() % 65);
        for (uint32_t j = 0; j < N / 4u; ++j) {
            const uint32_t r = rnd(), r2 = rnd();
            const int side = r & 1, n_in = (r >> 1) % 8 < 4 ? 4 : (int)((r >> 1) % 8) - 4;          // half of the words lie inside the row
            const int32_t class_mode = (int32_t)((r >> 4) % 3) - 1;
            const bool x_ist = (r >> 6) & 3;          // (three in four: b counts)
            const int32_t m = 200 + (int32_t)((r >> 8) % 16000);
            const uint32_t sx = pick_score(r2, (r2 >> 20) % 512);
            Partner y[4];
            uint32_t rr = r2 >> 3;
            for (int p = 0; p < 4; ++p) {
                const uint32_t t = 4u * j + (((uint32_t)p + (uint32_t)a) & 3u);
                const int32_t b = (int32_t)(t % 66u), ad = (int32_t)((t / 66u) % 128u);
                y[p].bound = std::min(255u, (t / (66u * 128u)) * bound_step);
                y[p].ist = (rr >> p) & 1 || (rr >> (4 + p)) & 1;          // (three in four)
                y[p].isq = b > 0;
                y[p].thr = b > 0 ? b - 1 : (int32_t)(rnd() % 65);
                y[p].len = side == 0 ? m + ad : m - ad;
                y[p].score = pick_score(rnd(), sx);
                y[p].role = (uint8_t)((y[p].ist ? 0x80 : 0) | b);
            }
            check_word(x_isq, x_ist, kx0, 64, m, sx, side, class_mode, n_in, y);
            words += 4;
        }
    }
    return words;
}

static unsigned long long caps()
{
    unsigned long long cases = 0;
    for (int32_t kcap : {0, 31, 63})
        for (int side = 0; side < 2; ++side)
            for (int32_t class_mode = -1; class_mode <= 1; ++class_mode)
                for (int n_in = 0; n_in <= 4; ++n_in)
                    for (int roles = 0; roles < 16; ++roles)
                        for (int32_t kx0 = 0; kx0 <= 64; ++kx0)
                            for (int rep = 0; rep < 24; ++rep) {
                                const bool x_isq = roles & 1, x_ist = roles & 2;
                                const int32_t m = 100 + (int32_t)(rnd() % 16000);
                                const uint32_t sx = pick_score(rnd(), rnd() % 512);
                                Partner y[4];
                                for (int p = 0; p < 4; ++p) {
                                    y[p].ist = p == 0 ? (roles & 4) != 0 : rnd() & 1;
                                    y[p].isq = p == 0 ? (roles & 8) != 0 : rnd() & 1;
                                    y[p].thr = (int32_t)(rnd() % 65);
                                    const int32_t ad = (int32_t)(rnd() % 3 == 0 ? rnd() % 64 : rnd() % (uint32_t)(kcap + 2));
                                    y[p].len = side == 0 ? m + ad : m - ad;
                                    y[p].bound = rnd() % 4 == 0 ? rnd() % 256 : rnd() % (uint32_t)(kcap + 3);
                                    y[p].score = pick_score(rnd(), sx);
                                    y[p].role = surv_role_byte(y[p].ist, y[p].isq, y[p].thr, kcap);
                                }
                                check_word(x_isq, x_ist, kx0, kcap, m, sx, side, class_mode, n_in, y);
                                ++cases;
                            }
    return cases;
}

// ---- whole rows through the staging arithmetic --------------------------------------------------------------------------------------
struct Log {
    uint32_t chunk, fill = 0, fill_n = 0, cand = 0, kept = 0;
    std::vector<uint32_t> st, events;          // events: writes (index, word) and flushes (class, words) in order
    explicit Log(uint32_t c) : chunk(c), st(c + 64) {}
    void put(uint32_t at, uint32_t word) { st.at(at) = word; events.push_back(at); events.push_back(word); }
    void flush(bool narrow)
    {
        events.push_back(narrow ? 0xfffffffeu : 0xffffffffu);
        const uint32_t cnt = narrow ? fill_n : fill;
        for (uint32_t i = 0; i < cnt; ++i) events.push_back(st.at(narrow ? (uint32_t)st.size() - 1u - i : i));
        if (narrow) fill_n = 0; else fill = 0;
    }
};

struct Row {
    bool x_isq, x_ist;
    int32_t kx0, kcap, m, class_mode;
    uint32_t sx;
    int side;
    std::vector<Partner> y;
};

static void stage(Log &L, uint32_t c0, const uint64_t (&am)[4], const uint64_t (&an)[4])
{
    // the lanes of a write store in any order on the device; here in the order of the lanes, which makes the logs comparable
    surv_batch(am, an, L.fill, L.fill_n, L.chunk,
               [&](uint64_t lanes, uint32_t off_a, uint32_t off_n) {
                   for (int lane = 0; lane < 64; ++lane) {
                       if (surv_lane_bit(lanes, lane) == 0) continue;
                       uint32_t at_a = off_a + surv_rank(am, lane), at_n = (uint32_t)L.st.size() - 1u - (off_n + surv_rank(an, lane));
                       for (int b = 0; b < 4; ++b) {
                           const uint32_t ka = surv_lane_bit(am[b], lane), kn = surv_lane_bit(an[b], lane);
                           if (ka | kn) L.put(ka ? at_a : at_n, c0 + 4u * (uint32_t)lane + (uint32_t)b);
                           at_a += ka;
                           at_n -= kn;
                       }
                   }
               },
               [&](bool narrow) { L.flush(narrow); });
}

static void scan_single(Log &L, const Row &R)
{
    const uint32_t len = (uint32_t)R.y.size();
    for (uint32_t c0 = 0; c0 < len; c0 += SURV_BATCH) {
        uint64_t am[4] = {0, 0, 0, 0}, an[4] = {0, 0, 0, 0};
        for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < 4; ++b) {
                const uint32_t e = c0 + 4u * (uint32_t)lane + (uint32_t)b;
                const Partner &y = R.y[e < len ? e : len - 1u];
                const SurvTest t = surv_test(e < len, R.x_isq, R.x_ist, y.isq, y.ist, R.kx0, y.thr, R.kcap, R.m, y.len, y.bound, R.sx, y.score, R.side, R.class_mode);
                L.cand += t.cand;
                L.kept += t.accept;
                if (t.keep && !t.to_narrow) am[b] |= (uint64_t)1 << lane;
                if (t.to_narrow) an[b] |= (uint64_t)1 << lane;
            }
        stage(L, c0, am, an);
    }
}

static void scan_packed(Log &L, const Row &R)
{
    constexpr int U = 4;
    const uint32_t len = (uint32_t)R.y.size();
    const SurvX X = surv_x(R.x_isq, R.x_ist, R.kx0, R.kcap, R.m, R.sx, R.side, R.class_mode);
    for (uint32_t c0 = 0; c0 < len; c0 += SURV_BATCH * U) {
        uint32_t keep[U][64], role[U][64];
        bool any = false;
        for (int u = 0; u < U; ++u)
            for (int lane = 0; lane < 64; ++lane) {
                const uint32_t e0 = c0 + (uint32_t)SURV_BATCH * (uint32_t)u + 4u * (uint32_t)lane;
                uint32_t bound = 0, rl = 0, len7 = 0, s01 = 0, s23 = 0;
                for (int p = 0; p < 4; ++p) {
                    const Partner &y = R.y[e0 + (uint32_t)p < len ? e0 + (uint32_t)p : len - 1u];
                    bound |= y.bound << (8 * p);
                    rl |= (uint32_t)y.role << (8 * p);
                    len7 |= (uint32_t)surv_len_byte((uint32_t)y.len) << (8 * p);
                    (p < 2 ? s01 : s23) |= (uint32_t)surv_score_half(y.score) << (16 * (p & 1));
                }
                rl &= surv_inr_bytes((int32_t)len - (int32_t)e0);
                uint32_t cand, accept;
                if (R.side == 0) surv_test4<0>(X, bound, rl, len7, s01, s23, cand, accept, keep[u][lane]);
                else surv_test4<1>(X, bound, rl, len7, s01, s23, cand, accept, keep[u][lane]);
                role[u][lane] = rl;
                L.cand += (uint32_t)__builtin_popcount(cand);
                L.kept += (uint32_t)__builtin_popcount(accept);
                any = any || keep[u][lane] != 0;
            }
        if (!any) continue;
        for (int u = 0; u < U; ++u) {
            uint64_t am[4] = {0, 0, 0, 0}, an[4] = {0, 0, 0, 0};
            bool any_u = false;
            for (int lane = 0; lane < 64; ++lane) {
                const uint32_t kn = keep[u][lane] & surv_narrow4(X, role[u][lane]), ka = keep[u][lane] & ~kn;
                any_u = any_u || keep[u][lane] != 0;
                for (int b = 0; b < 4; ++b) {
                    if (ka & (0x80u << (8 * b))) am[b] |= (uint64_t)1 << lane;
                    if (kn & (0x80u << (8 * b))) an[b] |= (uint64_t)1 << lane;
                }
            }
            if (any_u) stage(L, c0 + (uint32_t)SURV_BATCH * (uint32_t)u, am, an);
        }
    }
}

static unsigned long long n_rows = 0, n_chunks = 0, n_kept = 0;

static bool one_row(uint32_t chunk, uint32_t len, int keep_mix, int side, int32_t class_mode, uint32_t have)
{
    Row R;
    R.side = side;
    R.class_mode = class_mode;
    R.kcap = keep_mix == 3 ? 31 : 63;
    R.x_isq = rnd() % 8 != 0;
    R.x_ist = rnd() % 8 != 0;
    R.kx0 = (int32_t)(keep_mix == 1 ? 20 + rnd() % 20 : rnd() % 65);          // (mix 1: thresholds on both sides of 31)
    R.m = 300 + (int32_t)(rnd() % 4000);
    R.sx = pick_score(rnd(), 100 + rnd() % 300);
    R.y.resize(len);
    for (Partner &y : R.y) {
        y.ist = rnd() % 8 != 0;
        y.isq = rnd() % 8 != 0;
        y.thr = (int32_t)(keep_mix == 1 ? 20 + rnd() % 20 : rnd() % 65);
        const int32_t ad = (int32_t)(rnd() % (keep_mix == 0 ? 64u : 12u));
        y.len = side == 0 ? R.m + ad : R.m - ad;
        y.bound = keep_mix == 0 ? rnd() % 256 : keep_mix == 2 ? rnd() % 8 : rnd() % 48;          // (mix 0: few pairs kept; 2: nearly all)
        y.score = keep_mix == 2 && rnd() % 16 ? 0u : pick_score(rnd(), R.sx);
        y.role = surv_role_byte(y.ist, y.isq, y.thr, R.kcap);
    }
    Log A(chunk), B(chunk);
    const uint32_t n = have ? rnd() % (have + 1) : 0u;
    for (Log *L : {&A, &B}) {
        for (uint32_t i = 0; i < have - n; ++i) L->st[i] = 0x40000000u + i;
        for (uint32_t i = 0; i < n; ++i) L->st[L->st.size() - 1 - i] = 0x80000000u + i;
        L->fill = have - n;
        L->fill_n = n;
    }
    scan_single(A, R);
    scan_packed(B, R);
    ++n_rows;
    n_kept += A.kept;
    for (uint32_t e : A.events) n_chunks += e >= 0xfffffffeu;
    const bool ok = A.events == B.events && A.fill == B.fill && A.fill_n == B.fill_n && A.cand == B.cand && A.kept == B.kept && A.st == B.st;
    if (!ok) fprintf(stderr, "row mismatch: chunk %u len %u mix %d side %d mode %d have %u: fill %u + %u against %u + %u, kept %u against %u\n", chunk, len, keep_mix, side, class_mode, have, A.fill, A.fill_n, B.fill, B.fill_n, A.kept, B.kept);
    return ok;
}

int main(int argc, char **argv)
{
    const bool quick = argc > 1 && strcmp(argv[1], "quick") == 0;
    const unsigned long long words = sweep(quick ? 15u : 1u);
    const unsigned long long cases = caps();
    bool ok = n_fail == 0;
    std::vector<uint32_t> lens = {0, 1, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025};
    for (uint32_t l = 2047; l <= 2305; l += quick ? 7 : 1) lens.push_back(l);
    for (uint32_t chunk : {2048u, 256u})
        for (uint32_t len : lens)
            for (int mix = 0; mix < 4; ++mix)
                for (int side = 0; side < 2; ++side)
                    ok = one_row(chunk, len, mix, side, (len + (uint32_t)mix) % 4 == 0 ? -1 : 0, (mix + side) % 2 ? rnd() % chunk : 0u) && ok;
    if (!ok) return 1;
    if (n_chunks == 0 || n_kept == 0) { fprintf(stderr, "nothing kept or no chunk left\n"); return 2; }
    printf("ok %llu %llu %llu %llu %llu\n", words, cases, n_rows, n_chunks, n_kept);
    return 0;
}
