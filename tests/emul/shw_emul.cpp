// CPU emulation of the prefix ("SHW") tiles of isocon_amd/csrc/shw.hpp, lane by lane, on the SAME lane-level math header (hw_core.hpp,
// modes PREFIX_LOCATE and PREFIX_ENDS) and the same cut rule (hw_plan.hpp, HwPrefixCut): lets the not-gpu suite check both modes against
// the plain restatement of tests/shw_cases.py.  Test infrastructure.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../isocon_amd/csrc/hw_plan.hpp"

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

struct Query {
    const char *q;
    int P, nl;
    const char **ts;
    const int *tl;
    Packed Q;
    std::vector<Packed> T;
};

// One tile (lanes: indices into the query's targets) of W words with thresholds thr.  MODE PREFIX_LOCATE: out_h / out_end; PREFIX_ENDS
// (thr = the distances): out_cnt and at most cap ends per lane at out_ends[cap * lane ..].  A band that does not fit: -3 in out_h / out_cnt.
template <int W, int MODE>
static void tile(Query &X, const std::vector<uint32_t> &lanes, const int *thr, int cap, int32_t *out_h, int32_t *out_end, int32_t *out_cnt, int32_t *out_ends)
{
    const int P = X.P;
    auto qlo = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)X.Q.lo.size() ? X.Q.lo[ci] : 0; };
    auto qhi = [&](int ci) -> uint64_t { return ci >= 0 && ci < (int)X.Q.hi.size() ? X.Q.hi[ci] : 0; };
    auto f_lo = [&](int32_t off) { return stream64(qlo, off); };
    auto f_hi = [&](int32_t off) { return stream64(qhi, off); };
    auto alone = [](bool live) { return live; };
    int kmax = -1, cmax = 0;
    for (uint32_t l : lanes) {
        kmax = std::max(kmax, thr[l]);
        cmax = std::max(cmax, std::min(X.tl[l], P + thr[l]));
    }
    if (kmax < 0) return;
    if (2 * kmax + 1 > 64 * W) {
        for (uint32_t l : lanes) (MODE == HW_PREFIX_LOCATE ? out_h : out_cnt)[l] = -3;
        return;
    }
    HwTile A; A.P = P; A.a0 = -kmax; A.ncols_max = cmax; A.jx = std::max(1, P - kmax);
    for (uint32_t l : lanes) {
        HwLane ln; memset(&ln, 0, sizeof ln);
        ln.ncols = std::min(X.tl[l], P + thr[l]); ln.k = thr[l]; ln.h = MODE == HW_PREFIX_ENDS ? thr[l] : 0;
        const Packed &T = X.T[l];
        auto text = [&](int32_t jb, uint32_t &wl, uint32_t &wh) {
            wl = wh = 0;
            for (int x = 0; x < 32; ++x) { wl |= T.bit(T.lo, jb + x) << x; wh |= T.bit(T.hi, jb + x) << x; }
        };
        int c = 0;
        auto sink = [&](int32_t end, int, uint64_t, uint64_t) {
            if (c < cap) out_ends[(size_t)cap * l + c] = end;
            ++c;
        };
        hw_run<W, MODE>(A, ln, f_lo, f_hi, text, alone, sink);
        if (MODE == HW_PREFIX_LOCATE) {
            if (ln.r_h <= thr[l]) { out_h[l] = ln.r_h; out_end[l] = ln.r_end; }
        } else out_cnt[l] = c;
    }
}

// the tiles of the lanes with a threshold (>= 0) that need a kernel, by the host's cut under HwPrefixCut; out_w[l] = words of the lane's tile
template <int W, int MODE>
static void stage(Query &X, const int *thr, int cap, int32_t *out_h, int32_t *out_end, int32_t *out_cnt, int32_t *out_ends, int32_t *out_w)
{
    std::vector<uint32_t> idx, qs(X.nl, 0);
    for (int l = 0; l < X.nl; ++l)
        if (X.P > 0 && X.tl[l] > 0 && thr[l] >= 0 && X.tl[l] - X.P >= -thr[l]) idx.push_back((uint32_t)l);
    HwTiles tiles;
    hw_build_tiles(idx, qs.data(), 1, HwPrefixCut{thr}, tiles);
    for (int c = 0; c < 4; ++c) {
        const std::vector<uint32_t> &lp = tiles.lane_pair[c];
        for (size_t t0 = 0; t0 < lp.size(); t0 += 64) {
            std::vector<uint32_t> lanes;
            for (size_t i = t0; i < t0 + 64 && i < lp.size(); ++i) if (lp[i] != 0xffffffffu) lanes.push_back(lp[i]);
            if (out_w) for (uint32_t l : lanes) out_w[l] = 1 << c;
            tile<W, MODE>(X, lanes, thr, cap, out_h, out_end, out_cnt, out_ends);
        }
    }
}

// LOCATE on every lane with thr[l] >= 0 (out_h / out_end, -1: no hit or no kernel), then ENDS on the hits with their distances (out_cnt,
// out_ends), every tile run on W words whatever its class is (out_w[l]: the words of the lane's LOCATE tile, 0: no kernel).
template <int W>
static void query(Query &X, const int *thr, int cap, int32_t *out_h, int32_t *out_end, int32_t *out_cnt, int32_t *out_ends, int32_t *out_w)
{
    for (int l = 0; l < X.nl; ++l) { out_h[l] = -1; out_end[l] = -1; out_cnt[l] = 0; out_w[l] = 0; }
    stage<W, HW_PREFIX_LOCATE>(X, thr, cap, out_h, out_end, out_cnt, out_ends, out_w);
    std::vector<int> hs(X.nl);
    for (int l = 0; l < X.nl; ++l) hs[l] = out_h[l] >= 0 ? out_h[l] : -1;
    stage<W, HW_PREFIX_ENDS>(X, hs.data(), cap, out_h, out_end, out_cnt, out_ends, nullptr);
}

extern "C" void emul_shw_query(int W, const char *q, int P, int nl, const char **ts, const int *tl, const int *thr, int cap, int32_t *out_h, int32_t *out_end,
                               int32_t *out_cnt, int32_t *out_ends, int32_t *out_w)
{
    Query X;
    X.q = q; X.P = P; X.nl = nl; X.ts = ts; X.tl = tl;
    X.Q.set(q, P);
    X.T.resize(nl);
    for (int l = 0; l < nl; ++l) X.T[l].set(ts[l], tl[l]);
    switch (W) {
    case 1: query<1>(X, thr, cap, out_h, out_end, out_cnt, out_ends, out_w); break;
    case 2: query<2>(X, thr, cap, out_h, out_end, out_cnt, out_ends, out_w); break;
    case 4: query<4>(X, thr, cap, out_h, out_end, out_cnt, out_ends, out_w); break;
    case 8: query<8>(X, thr, cap, out_h, out_end, out_cnt, out_ends, out_w); break;
    default: for (int l = 0; l < nl; ++l) out_h[l] = -99;
    }
}
