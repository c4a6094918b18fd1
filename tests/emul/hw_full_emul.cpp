// CPU emulation of one wavefront (one pair) of the un-banded infix kernels (isocon_amd/csrc/hw_full.hpp): 64 lanes in lock step on
// the SAME lane-level math header (hw_full_core.hpp) -- systolic column loop, passes of 64 blocks with the 2-bit boundary buffer,
// the [step][lane] trace store, the walk and the trailing run.  Test infrastructure for the not-gpu suite.
#include <cstring>
#include <vector>
#include "../../isocon_amd/csrc/hw_full_core.hpp"

using namespace isocon;

static inline int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

struct Planes {
    std::vector<uint64_t> lo, hi;
    int len = 0;
    void set(const char *s, int n)
    {
        len = n;
        const int nc = (n + 63) / 64 + 1;
        lo.assign(nc, 0); hi.assign(nc, 0);
        for (int i = 0; i < n; ++i) {
            const int c = code_of(s[i]);
            if (c & 1) lo[i >> 6] |= (uint64_t)1 << (i & 63);
            if (c & 2) hi[i >> 6] |= (uint64_t)1 << (i & 63);
        }
    }
    int base(long p) const { return (p < 0 || p >= len) ? 0 : (int)((lo[p >> 6] >> (p & 63)) & 1) | (int)(((hi[p >> 6] >> (p & 63)) & 1) << 1); }
};

struct Unit { uint64_t pv, ph; };

// One pass sequence (all passes of 64 blocks) of one mode.  text(c) = base of 0-based column c.  Results of the query's last row.
template <int MODE, class Text>
static void run(const Planes &Q, int32_t m, int32_t ncols, int32_t h, Text text, Unit *trace, uint64_t *fin, int32_t ms,
                int32_t &r_score, int32_t &r_best, int32_t &r_col)
{
    auto qlo = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.lo.size() ? Q.lo[ci] : 0; };
    auto qhi = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.hi.size() ? Q.hi[ci] : 0; };
    const int32_t passes = hwf_passes(m);
    std::vector<uint32_t> bound(hwf_bound_words(ncols) + 1, 0);
    for (int32_t pass = 0; pass < passes; ++pass) {
        const int32_t nbl = hwf_pass_lanes(m, pass);
        HwfLane L[64];
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
                    hin = pass == 0 ? (MODE == HWF_LOCATE ? 0 : 1) : (s < ncols ? hwf_bound_get(bound[s >> 4], s) : 0);
                } else {
                    ch = hwf_packed_base(packed[l - 1]);
                    hin = hwf_packed_delta(packed[l - 1]);
                }
                const int32_t col = s - l;
                int32_t hout = 0;
                if (col >= 0 && col < ncols && l < nbl) {
                    uint64_t ph;
                    hout = hwf_step<MODE>(L[l], ch, hin, col, h, ph);
                    if (MODE == HWF_TRACE) {
                        if (trace) trace[hwf_trace_unit(m, ms, pass * 64 + l, col + 1)] = Unit{L[l].Pv, ph};
                        if (col == ncols - 1) fin[pass * 64 + l] = L[l].Pv;
                    }
                    if (l == 63 && pass + 1 < passes) {
                        bw = hwf_bound_add(bw, col, hout);
                        if (hwf_bound_full(col, ncols)) { bound[col >> 4] = bw; bw = 0; }
                    }
                }
                next[l] = hwf_pack(ch, hout);
            }
            memcpy(packed, next, sizeof packed);
        }
        if (pass == passes - 1) {
            const int lstar = ((m - 1) >> 6) - pass * 64;
            r_score = L[lstar].score; r_best = L[lstar].best; r_col = L[lstar].best_col;
        }
    }
}

extern "C" void emul_hw_full_pair(const char *q, int m, const char *t, int n, int k, int32_t *out)
{
    out[0] = -1; out[1] = -1; out[2] = -1; out[3] = 0; out[4] = 0;
    if (m <= 0 || n <= 0 || k < 0 || n - m < -k) return;
    Planes Q, T;
    Q.set(q, m); T.set(t, n);
    int32_t sc, best, col;
    run<HWF_LOCATE>(Q, m, n, 0, [&](int32_t c) { return T.base(c); }, nullptr, nullptr, 0, sc, best, col);
    if (best > k) return;
    const int32_t h = best, end = col;
    const int32_t nc = end + 1 < m + h ? end + 1 : m + h;
    run<HWF_START>(Q, m, nc, h, [&](int32_t c) { return T.base((long)end - c); }, nullptr, nullptr, 0, sc, best, col);
    if (col < 0) { out[0] = -4; return; }
    const int32_t start = end - col, ms = end - start + 1;
    std::vector<Unit> trace(start == 0 ? hwf_trace_units(m, ms) : 0);
    std::vector<uint64_t> fin(hwf_blocks(m), 0);
    run<HWF_TRACE>(Q, m, ms, h, [&](int32_t c) { return T.base((long)start + c); }, start == 0 ? trace.data() : nullptr, fin.data(), ms, sc, best, col);
    if (sc != h) { out[0] = -5; return; }
    out[0] = h; out[1] = start; out[2] = end;
    out[4] = hwf_trail(m, [&](int32_t b) { return fin[b]; });
    // (only start == 0 can have a leading insertion run: hw.hpp)
    if (start == 0) out[3] = hwf_walk(m, ms, [&](int32_t b, int32_t j, uint64_t &pv, uint64_t &ph) { const Unit &u = trace[hwf_trace_unit(m, ms, b, j)]; pv = u.pv; ph = u.ph; });
}

// the pass boundary at small sizes: the same pair with the trace layout's arithmetic only (units never overlap, all inside the store)
extern "C" int emul_hw_full_layout_ok(int m, int ms)
{
    const uint64_t total = hwf_trace_units(m, ms);
    std::vector<char> seen(total, 0);
    for (int b = 0; b < hwf_blocks(m); ++b)
        for (int j = 1; j <= ms; ++j) {
            const uint64_t u = hwf_trace_unit(m, ms, b, j);
            if (u < hwf_fin_units(m) || u >= total || seen[u]) return 0;
            seen[u] = 1;
        }
    return 1;
}
