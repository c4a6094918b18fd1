// What tests/emul/hw_rows_emul.cpp and tests/emul/hw_full_ends_emul.cpp share: 2-bit planes of a string, one wavefront of the un-banded
// infix kernels (isocon_amd/csrc/hw_full.hpp hwf_run: 64 lanes in lock step on hw_full_core.hpp, with the sink of mode ENDS), the
// un-banded START of one (pair, end) entry (k_hwl_starts_full of hw_rows.hpp) and the programs' line protocol:
//   in:  <query> <target> <k>            ("-": the empty string)
//   out: <h or -1> <ends counted> <first end or -1> <ends listed> then <start> <end> per listed end
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../isocon_amd/csrc/hw_full_core.hpp"
#include "../../isocon_amd/csrc/hw_rows_core.hpp"

using namespace isocon;

static inline int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

struct Planes {
    std::vector<uint64_t> lo, hi;
    int len = 0;
    void set(const std::string &s)
    {
        len = (int)s.size();
        const int nc = (len + 63) / 64 + 1;
        lo.assign(nc, 0); hi.assign(nc, 0);
        for (int i = 0; i < len; ++i) {
            const int c = code_of(s[i]);
            if (c & 1) lo[i >> 6] |= (uint64_t)1 << (i & 63);
            if (c & 2) hi[i >> 6] |= (uint64_t)1 << (i & 63);
        }
    }
    int base(long p) const { return (p < 0 || p >= len) ? 0 : (int)((lo[p >> 6] >> (p & 63)) & 1) | (int)(((hi[p >> 6] >> (p & 63)) & 1) << 1); }
};

// All passes of one mode, as hwf_run: text(c) = base of 0-based column c; sink(score, col) after every column of the query's last row.
template <int MODE, class Text, class Sink>
static void wave_run(const Planes &Q, int32_t m, int32_t ncols, int32_t h, Text text, Sink sink, int32_t &r_col)
{
    auto qlo = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.lo.size() ? Q.lo[ci] : 0; };
    auto qhi = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.hi.size() ? Q.hi[ci] : 0; };
    const int32_t passes = hwf_passes(m);
    std::vector<uint32_t> bound(hwf_bound_words(ncols) + 1, 0);
    r_col = -1;
    for (int32_t pass = 0; pass < passes; ++pass) {
        const int32_t nbl = hwf_pass_lanes(m, pass);
        std::vector<HwfLane> L(64);
        int32_t packed[64], next[64];
        for (int l = 0; l < 64; ++l) {
            const int32_t row0 = (pass * 64 + l) * 64;
            const uint64_t lo = MODE == HWF_START ? stream64_rev(qlo, m, row0) : stream64(qlo, row0);
            const uint64_t hi = MODE == HWF_START ? stream64_rev(qhi, m, row0) : stream64(qhi, row0);
            hwf_lane_init(L[l], lo, hi, m, row0);
            packed[l] = hwf_pack(0, 0);
        }
        uint32_t bw = 0;
        const int32_t steps = ncols + nbl - 1;
        for (int32_t s = 0; s < steps; ++s) {
            for (int l = 0; l < 64; ++l) {
                int32_t ch, hin;
                if (l == 0) {
                    ch = s < ncols ? text(s) : 0;
                    hin = pass == 0 ? (MODE == HWF_LOCATE || MODE == HWF_ENDS ? 0 : 1) : (s < ncols ? hwf_bound_get(bound[s >> 4], s) : 0);
                } else {
                    ch = hwf_packed_base(packed[l - 1]);
                    hin = hwf_packed_delta(packed[l - 1]);
                }
                const int32_t col = s - l;
                int32_t hout = 0;
                if (col >= 0 && col < ncols && l < nbl) {
                    uint64_t ph;
                    hout = hwf_step<MODE>(L[l], ch, hin, col, h, ph);
                    if (MODE == HWF_ENDS && pass * 64 + l == ((m - 1) >> 6)) sink(L[l].score, col);
                    if (l == 63 && pass + 1 < passes) {
                        bw = hwf_bound_add(bw, col, hout);
                        if (hwf_bound_full(col, ncols)) { bound[col >> 4] = bw; bw = 0; }
                    }
                }
                next[l] = hwf_pack(ch, hout);
            }
            memcpy(packed, next, sizeof packed);
        }
        if (pass == passes - 1) r_col = L[((m - 1) >> 6) - pass * 64].best_col;
    }
}

// the smallest start of distance h for `end`, or -4
static int32_t full_start(const Planes &Q, const Planes &T, int32_t m, int32_t h, int32_t end)
{
    const int32_t nc = end + 1 < m + h ? end + 1 : m + h;
    int32_t col;
    wave_run<HWF_START>(Q, m, nc, h, [&](int32_t c) { return T.base((long)end - c); }, [](int32_t, int32_t) {}, col);
    return col >= 0 ? end - col : -4;
}

// ends(Q, T, m, n, h, fill, C, listed): one run of the kernel under test -- count (fill false: C) or fill (h known: the ends into listed)
template <class Ends>
static int serve(Ends ends)
{
    char qb[1 << 16], tb[1 << 16];
    int k;
    while (scanf("%65535s %65535s %d", qb, tb, &k) == 3) {
        const std::string q = strcmp(qb, "-") ? qb : "", t = strcmp(tb, "-") ? tb : "";
        const int32_t m = (int32_t)q.size(), n = (int32_t)t.size();
        if (m <= 0 || n <= 0 || k < 0 || n - m < -k) { printf("-1 0 -1 0\n"); continue; }
        Planes Q, T;
        Q.set(q); T.set(t);
        HwrCount C;
        hwr_count_init(C);
        std::vector<int32_t> listed;
        ends(Q, T, m, n, 0, false, C, listed);
        if (C.best > k) { printf("-1 0 -1 0\n"); continue; }
        ends(Q, T, m, n, C.best, true, C, listed);
        printf("%d %u %d %zu", C.best, C.count, C.first, listed.size());
        for (int32_t e : listed) printf(" %d %d", full_start(Q, T, m, C.best, e), e);
        printf("\n");
    }
    return 0;
}
