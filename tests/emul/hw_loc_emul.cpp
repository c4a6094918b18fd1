// CPU emulation of the ENDS tile and the START tile of isocon_hw_locations (isocon_amd/csrc/hw_loc.hpp), lane by lane, on the SAME
// lane-level math header (hw_core.hpp): lets the not-gpu suite check the ENDS mode of hw_run and the per-end START pass against the plain
// restatement of tests/hw_locations_cases.py.  Test infrastructure.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../isocon_amd/csrc/hw_core.hpp"

using namespace isocon;

static inline int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

struct Packed {
    std::vector<uint64_t> lo, hi;
    void set(const char *s, int n)
    {
        const int nc = (n + 63) / 64 + 2;
        lo.assign(nc, 0); hi.assign(nc, 0);
        for (int i = 0; i < n; ++i) {
            const int c = code_of(s[i]);
            if (c & 1) lo[i >> 6] |= (uint64_t)1 << (i & 63);
            if (c & 2) hi[i >> 6] |= (uint64_t)1 << (i & 63);
        }
    }
    uint32_t bit(const std::vector<uint64_t> &v, long p) const { return (p < 0 || p >= (long)v.size() * 64) ? 0u : (uint32_t)(v[p >> 6] >> (p & 63)) & 1u; }
};

// One ENDS tile of WE words (lanes: the targets, hs[l] = the pair's distance, < 0: no hit, the lane stays empty), then one START tile of WS
// words over all (lane, end) entries.  out_cnt[l] = ends of lane l (-3: the tile's band does not fit); the entries of lane l start at
// cap * l in out_end / out_start (at most cap are written; out_start -3: band, -4: no start).
template <int WE, int WS>
static void tile(const char *q, int P, int nl, const char **ts, const int *tl, const int *hs, int cap, int32_t *out_cnt, int32_t *out_end, int32_t *out_start)
{
    Packed Q; Q.set(q, P);
    std::vector<Packed> T(nl);
    for (int l = 0; l < nl; ++l) T[l].set(ts[l], tl[l]);
    auto qlo = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.lo.size() ? Q.lo[ci] : 0; };
    auto qhi = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)Q.hi.size() ? Q.hi[ci] : 0; };
    auto f_lo = [&](int32_t off) { return stream64(qlo, off); };
    auto f_hi = [&](int32_t off) { return stream64(qhi, off); };
    auto r_lo = [&](int32_t off) { return stream64_rev(qlo, P, off); };
    auto r_hi = [&](int32_t off) { return stream64_rev(qhi, P, off); };
    auto alone = [](bool live) { return live; };
    auto nosink = [](int32_t, int, uint64_t, uint64_t) {};
    for (int l = 0; l < nl; ++l) out_cnt[l] = 0;
    // ---- ENDS ----
    int dmax = -(1 << 30), hmax = 0, mmax = 0;
    std::vector<char> valid(nl, 0);
    for (int l = 0; l < nl; ++l) {
        valid[l] = P > 0 && tl[l] > 0 && hs[l] >= 0 && tl[l] - P >= -hs[l];
        if (!valid[l]) continue;
        dmax = std::max(dmax, tl[l] - P); hmax = std::max(hmax, hs[l]); mmax = std::max(mmax, tl[l]);
    }
    if (dmax == -(1 << 30)) return;
    if (hw_locate_rows(dmax, hmax) > 64 * WE) { for (int l = 0; l < nl; ++l) if (valid[l]) out_cnt[l] = -3; return; }
    HwTile A; A.P = P; A.a0 = hw_locate_a0(dmax, hmax); A.ncols_max = mmax; A.jx = std::max(1, P - hmax);
    for (int l = 0; l < nl; ++l) {
        if (!valid[l]) continue;
        HwLane ln; memset(&ln, 0, sizeof ln);
        ln.ncols = tl[l]; ln.k = hs[l]; ln.h = hs[l];
        auto text = [&](int32_t jb, uint32_t &wl, uint32_t &wh) {
            wl = wh = 0;
            for (int x = 0; x < 32; ++x) { wl |= T[l].bit(T[l].lo, jb + x) << x; wh |= T[l].bit(T[l].hi, jb + x) << x; }
        };
        int c = 0;
        auto sink = [&](int32_t end, int, uint64_t, uint64_t) {
            if (c < cap) out_end[(size_t)cap * l + c] = end;
            ++c;
        };
        hw_run<WE, HW_ENDS>(A, ln, f_lo, f_hi, text, alone, sink);
        out_cnt[l] = c;
    }
    // ---- START of every entry ---- (reversed query against the reversed prefix t[0..end], band [-hmax, hmax])
    if (2 * hmax + 1 > 64 * WS) {
        for (int l = 0; l < nl; ++l) for (int c = 0; c < std::min(out_cnt[l], cap); ++c) out_start[(size_t)cap * l + c] = -3;
        return;
    }
    int cmax = 0;
    for (int l = 0; l < nl; ++l) for (int c = 0; c < std::min(out_cnt[l], cap); ++c) cmax = std::max(cmax, std::min(out_end[(size_t)cap * l + c] + 1, P + hmax));
    HwTile B; B.P = P; B.a0 = -hmax; B.ncols_max = cmax; B.jx = std::max(1, P - hmax);
    for (int l = 0; l < nl; ++l) {
        for (int c = 0; c < std::min(out_cnt[l], cap); ++c) {
            const long e = out_end[(size_t)cap * l + c];
            HwLane ln; memset(&ln, 0, sizeof ln);
            ln.ncols = std::min((int)e + 1, P + hmax); ln.k = hs[l]; ln.h = hs[l];
            auto text = [&](int32_t jb, uint32_t &wl, uint32_t &wh) {
                wl = wh = 0;
                for (int x = 0; x < 32; ++x) { wl |= T[l].bit(T[l].lo, e - jb - x) << x; wh |= T[l].bit(T[l].hi, e - jb - x) << x; }
            };
            hw_run<WS, HW_START>(B, ln, r_lo, r_hi, text, alone, nosink);
            out_start[(size_t)cap * l + c] = ln.r_pl < 1 ? -4 : (int32_t)(e - (ln.r_pl - 1));
        }
    }
}

template <int WE>
static void tile_ws(int WS, const char *q, int P, int nl, const char **ts, const int *tl, const int *hs, int cap, int32_t *out_cnt, int32_t *out_end, int32_t *out_start)
{
    switch (WS) {
    case 1: tile<WE, 1>(q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 2: tile<WE, 2>(q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 4: tile<WE, 4>(q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 8: tile<WE, 8>(q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    default: for (int l = 0; l < nl; ++l) out_cnt[l] = -99;
    }
}

extern "C" void emul_hw_loc_tile(int WE, int WS, const char *q, int P, int nl, const char **ts, const int *tl, const int *hs, int cap, int32_t *out_cnt,
                                 int32_t *out_end, int32_t *out_start)
{
    switch (WE) {
    case 1: tile_ws<1>(WS, q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 2: tile_ws<2>(WS, q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 4: tile_ws<4>(WS, q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    case 8: tile_ws<8>(WS, q, P, nl, ts, tl, hs, cap, out_cnt, out_end, out_start); break;
    default: for (int l = 0; l < nl; ++l) out_cnt[l] = -99;
    }
}
