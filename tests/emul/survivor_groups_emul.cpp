// The staging arithmetic of the survivor-list builder (isocon_amd/csrc/nn_surv_core.hpp: 256 row positions per batch, four per lane)
// against a restatement of the loop it replaced: 64 positions per step, one per lane, the chunk check behind every step.  A program of
// its own for tests/test_survivor_groups.py (g++, plain and with -fsanitize=undefined,address).
// Every case is a row of some length with random keep and class masks and a buffer that already holds some pairs; both loops stage
// the row's kept positions in a buffer of exactly chunk + 64 words (the sanitized build sees any index outside it) and hand over
// chunks.  Checked: the same chunks (class and contents, in order) at the same places, the same remainder of both classes, no live
// word of the buffer overwritten.  stdout: "ok <cases> <chunks> <chunks that left behind group 0> .. <group 3>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../isocon_amd/csrc/nn_surv_core.hpp"

using namespace isocon;

struct Chunk {
    bool narrow;
    uint32_t step;          // the 64-position step behind which it left
    std::vector<uint32_t> words;
    bool operator==(const Chunk &o) const { return narrow == o.narrow && step == o.step && words == o.words; }
};

struct Stage {
    uint32_t chunk, fill = 0, fill_n = 0;
    std::vector<uint32_t> st;          // chunk + 64 words, as NN_STAGE
    std::vector<uint8_t> live;
    std::vector<Chunk> out;
    bool clobbered = false;
    explicit Stage(uint32_t c) : chunk(c), st(c + 64), live(c + 64, 0) {}
    void put(uint32_t at, uint32_t word)
    {
        if (live.at(at)) clobbered = true;
        st.at(at) = word;
        live.at(at) = 1;
    }
    void put_a(uint32_t i, uint32_t word) { put(i, word); }
    void put_n(uint32_t i, uint32_t word) { put((uint32_t)st.size() - 1u - i, word); }
    // emit_chunk of the kernel: one class leaves
    void flush(bool narrow, uint32_t step)
    {
        Chunk c;
        c.narrow = narrow;
        c.step = step;
        const uint32_t cnt = narrow ? fill_n : fill;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t at = narrow ? (uint32_t)st.size() - 1u - i : i;
            if (!live.at(at)) clobbered = true;          // a word of the chunk that nobody wrote
            c.words.push_back(st.at(at));
            live.at(at) = 0;
        }
        out.push_back(c);
        if (narrow) fill_n = 0; else fill = 0;
    }
    void prefill(uint32_t a, uint32_t n)
    {
        for (uint32_t i = 0; i < a; ++i) put_a(i, 0x40000000u + i);
        for (uint32_t i = 0; i < n; ++i) put_n(i, 0x80000000u + i);
        fill = a;
        fill_n = n;
    }
    std::vector<uint32_t> rest() const
    {
        std::vector<uint32_t> r;
        for (uint32_t i = 0; i < fill; ++i) r.push_back(st[i]);
        for (uint32_t i = 0; i < fill_n; ++i) r.push_back(st[st.size() - 1 - i]);
        return r;
    }
};

// cls[e]: 0 = not kept, 1 = 64-row class, 2 = 32-row class

// the loop as it was: 64 positions per step, lane = position
static void scan_steps(Stage &S, const std::vector<uint8_t> &cls)
{
    const uint32_t len = (uint32_t)cls.size();
    for (uint32_t c0 = 0; c0 < len; c0 += 64) {
        uint64_t am = 0, an = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t e = c0 + lane;
            if (e < len && cls[e] == 1) am |= (uint64_t)1 << lane;
            if (e < len && cls[e] == 2) an |= (uint64_t)1 << lane;
        }
        if ((am | an) == 0) continue;
        for (int lane = 0; lane < 64; ++lane) {
            const uint64_t lt = ((uint64_t)1 << lane) - 1;
            if (am >> lane & 1) S.put_a(S.fill + (uint32_t)__builtin_popcountll(am & lt), c0 + lane);
            if (an >> lane & 1) S.put_n(S.fill_n + (uint32_t)__builtin_popcountll(an & lt), c0 + lane);
        }
        S.fill += (uint32_t)__builtin_popcountll(am);
        S.fill_n += (uint32_t)__builtin_popcountll(an);
        if (S.fill + S.fill_n >= S.chunk) S.flush(S.fill_n > S.fill, c0 / 64);
    }
}

// the loop as the kernel runs it: 256 positions per batch, lane l = positions 4 l .. 4 l + 3
static void scan_batches(Stage &S, const std::vector<uint8_t> &cls)
{
    const uint32_t len = (uint32_t)cls.size();
    for (uint32_t c0 = 0; c0 < len; c0 += SURV_BATCH) {
        uint64_t am[SURV_PER_LANE] = {0, 0, 0, 0}, an[SURV_PER_LANE] = {0, 0, 0, 0};
        for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < SURV_PER_LANE; ++b) {
                const uint32_t e = c0 + 4u * lane + b;
                if (e < len && cls[e] == 1) am[b] |= (uint64_t)1 << lane;
                if (e < len && cls[e] == 2) an[b] |= (uint64_t)1 << lane;
            }
        uint32_t group = 0;          // (the callbacks come in the order of the groups: the step of a flush is that of the last write)
        surv_batch(am, an, S.fill, S.fill_n, S.chunk,
                   [&](uint64_t lanes, uint32_t off_a, uint32_t off_n) {
                       for (int lane = 0; lane < 64; ++lane) {
                           if (surv_lane_bit(lanes, lane) == 0) continue;
                           group = (uint32_t)lane / 16;
                           uint32_t at_a = off_a + surv_rank(am, lane), at_n = off_n + surv_rank(an, lane);
                           for (int b = 0; b < SURV_PER_LANE; ++b) {
                               const uint32_t ka = surv_lane_bit(am[b], lane), kn = surv_lane_bit(an[b], lane);
                               if (ka) S.put_a(at_a, c0 + 4u * lane + b);
                               if (kn) S.put_n(at_n, c0 + 4u * lane + b);
                               at_a += ka;
                               at_n += kn;
                           }
                       }
                   },
                   [&](bool narrow) { S.flush(narrow, c0 / 64 + group); });
    }
}

static unsigned long long n_cases = 0, n_chunks = 0, by_group[4] = {0, 0, 0, 0};

static bool one_case(uint32_t chunk, const std::vector<uint8_t> &cls, uint32_t fill, uint32_t fill_n)
{
    Stage A(chunk), B(chunk);
    A.prefill(fill, fill_n);
    B.prefill(fill, fill_n);
    scan_steps(A, cls);
    scan_batches(B, cls);
    ++n_cases;
    n_chunks += A.out.size();
    for (const Chunk &c : A.out) ++by_group[c.step % 4];
    const bool ok = !A.clobbered && !B.clobbered && A.out == B.out && A.fill == B.fill && A.fill_n == B.fill_n && A.rest() == B.rest();
    if (!ok)
        fprintf(stderr, "mismatch: chunk %u len %zu fill %u fill_n %u: %zu chunks against %zu, rest %u + %u against %u + %u, clobbered %d %d\n", chunk, cls.size(), fill, fill_n,
                A.out.size(), B.out.size(), A.fill, A.fill_n, B.fill, B.fill_n, (int)A.clobbered, (int)B.clobbered);
    return ok;
}

int main()
{
    std::mt19937 rng(20240607u);
    std::vector<uint32_t> lens = {0, 1, 3, 4, 63, 64, 65, 255, 256, 257};
    for (uint32_t l = 2047; l <= 2305; ++l) lens.push_back(l);
    const double keep_p[] = {0.0, 0.03, 0.4, 0.9, 1.0}, narrow_p[] = {0.0, 0.5, 1.0, 0.1};
    bool ok = true;
    for (uint32_t chunk : {2048u, 256u}) {
        // random rows: every length, every keep rate and class mix, a buffer that holds anything below a chunk
        for (uint32_t len : lens)
            for (double kp : keep_p)
                for (double np : narrow_p)
                    for (int rep = 0; rep < 2; ++rep) {
                        std::vector<uint8_t> cls(len);
                        for (auto &c : cls) c = (rng() % 10000) < kp * 10000 ? ((rng() % 10000) < np * 10000 ? 2 : 1) : 0;
                        const uint32_t have = rep == 0 ? 0u : rng() % chunk, n = have ? rng() % (have + 1) : 0u;
                        ok = one_case(chunk, cls, have - n, n) && ok;
                    }
        // a buffer that reaches the chunk inside each of the four groups of the first batch, with every margin, for both classes and a mix
        for (int group = 0; group < 4; ++group)
            for (uint32_t margin = 1; margin <= 64; ++margin)
                for (int mix = 0; mix < 3; ++mix) {
                    std::vector<uint8_t> cls(257 + 64 * group);
                    for (size_t e = 0; e < cls.size(); ++e) cls[e] = mix == 0 ? 1 : mix == 1 ? 2 : 1 + (uint8_t)(rng() & 1);
                    const uint32_t have = chunk - 64u * group - margin, n = mix == 0 ? have / 3 : mix == 1 ? have - have / 3 : rng() % (have + 1);
                    ok = one_case(chunk, cls, have - n, n) && ok;
                }
    }
    if (!ok) return 1;
    if (by_group[0] == 0 || by_group[1] == 0 || by_group[2] == 0 || by_group[3] == 0) { fprintf(stderr, "a group never flushed\n"); return 2; }
    printf("ok %llu %llu %llu %llu %llu %llu\n", n_cases, n_chunks, by_group[0], by_group[1], by_group[2], by_group[3]);
    return 0;
}
