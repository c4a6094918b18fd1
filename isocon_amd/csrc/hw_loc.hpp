// hw_loc.hpp -- every best location of an infix ("HW") pair: device side of isocon_hw_locations, what edlib.align(q, t, mode="HW",
// task="path") lists in `locations` -- every end column whose last-row value equals the distance, ascending, each with the smallest
// start of that distance.  Lane-level math: hw_core.hpp (modes ENDS and START); tiles as in hw.hpp: one wavefront = one shared query x
// up to 64 lanes.  After k_hw_locate (distance h and first end of every pair):
//   k_hw_loc_prep      thr[p] = h or -1 -- the threshold of the ENDS tiles and the caller's out_ed --, cnt[p] = 0
//   k_hw_ends<W, 0>    ENDS on the hits, tiles built with threshold h: cnt[p] = ends of pair p
//   (exclusive scan of cnt -> loc_ptr; its total sizes the output)
//   k_hw_ends<W, 1>    the same run again, end i of pair p written to slot loc_ptr[p] + i of the EXPANDED list: one entry per (pair, end)
//                      with the pair's query, target and distance -- the pair list of the START tiles
//   k_hw_starts<W>     the START pass of k_hw_finish alone on the expanded list, band [-h, h]: locs[2 slot] = start, locs[2 slot + 1] = end
// Two runs of ENDS instead of one into bounded per-lane lists: the count is exact, a pair may have as many ends as its target has columns
// (q all A in t all C) without a list bound to tune or an overflow run, and both runs produce a pair's ends in the order of its columns.
#pragma once
#include "common.hpp"
#include "hw.hpp"

namespace isocon {

__global__ __launch_bounds__(256) void k_hw_loc_prep(const int32_t *__restrict__ he, unsigned long long n_pairs, int32_t *__restrict__ thr, uint32_t *__restrict__ cnt)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    thr[p] = he[p * 2];
    cnt[p] = 0;
}

// the expanded list: one entry per (pair, end)
struct HwLocList {
    uint32_t *q, *t;     // query and target of the entry's pair
    int32_t *h;          // its distance: the threshold of the START tiles
    int32_t *he;         // [2 i] = h, [2 i + 1] = end
};

// in.pk = thr (k_hw_loc_prep): the tiles hold hits only.  FILL = 0: cnt[pair] = ends; FILL = 1: the entries loc_ptr[pair] .. of E.
template <int W, int FILL>
__global__ __launch_bounds__(256) void k_hw_ends(DevStore S, HwTileIn in, uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ loc_ptr, HwLocList E)
{
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= in.n_tiles) return;
    const uint32_t tile = in.tile_list ? (uint32_t)uniform_i32((int32_t)in.tile_list[slot]) : slot;
    const uint32_t q = (uint32_t)uniform_i32((int32_t)in.tile_q[tile]);
    const int32_t P = uniform_i32(S.lens[q]);
    const uint32_t pair = in.lane_pair[(size_t)tile * 64 + lane];
    const bool has = pair != 0xffffffffu;
    const uint32_t tid = has ? in.pt[pair] : q;
    const int32_t h = has ? in.pk[pair] : -1;
    const int32_t m = S.lens[tid];
    const bool valid = has && P > 0 && m > 0 && h >= 0 && m - P >= -h;
    const int32_t dmax = uniform_i32(wave_max_i32(valid ? m - P : -(1 << 30)));
    const int32_t hmax = uniform_i32(wave_max_i32(valid ? h : 0));
    const int32_t mmax = uniform_i32(wave_max_i32(valid ? m : 0));
    int32_t status = 0;
    uint32_t c = 0;
    if (dmax > -(1 << 30)) {
        if (hw_locate_rows(dmax, hmax) > 64 * W) status = -3;
        else {
            HwTile T;
            T.P = P; T.a0 = hw_locate_a0(dmax, hmax); T.ncols_max = mmax; T.jx = P - hmax > 1 ? P - hmax : 1;
            HwLane ln;
            ln.ncols = valid ? m : 0; ln.k = h; ln.h = h;
            const uint64_t *planes = S.planes;
            const uint32_t nseq = S.n;
            const int32_t nchunks = (int32_t)S.nchunks;
            auto chunk_lo = [&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + q) * 2] : 0; };
            auto chunk_hi = [&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + q) * 2 + 1] : 0; };
            auto plo = [&](int32_t off) { return stream64(chunk_lo, off); };
            auto phi = [&](int32_t off) { return stream64(chunk_hi, off); };
            const ulonglong2 *P2 = reinterpret_cast<const ulonglong2 *>(planes);
            ulonglong2 tcur = {0, 0};
            auto text = [&](int32_t jb, uint32_t &wl, uint32_t &wh) {
                if ((jb & 63) == 0) tcur = P2[(size_t)(jb >> 6) * nseq + tid];       // columns <-> target positions, 64 per load
                wl = (uint32_t)((jb & 32) ? (tcur.x >> 32) : tcur.x);
                wh = (uint32_t)((jb & 32) ? (tcur.y >> 32) : tcur.y);
            };
            auto any_live = [](bool live) { return __ballot(live) != 0; };
            const unsigned long long base = FILL && valid ? loc_ptr[pair] : 0;
            const unsigned long long room = FILL && valid ? loc_ptr[pair + 1] - base : 0;          // (what the count run found: never written past)
            auto sink = [&](int32_t end, int, uint64_t, uint64_t) {
                if (FILL && c < room) {
                    const unsigned long long i = base + c;
                    E.q[i] = q; E.t[i] = tid; E.h[i] = h;
                    E.he[i * 2] = h; E.he[i * 2 + 1] = end;
                }
                ++c;
            };
            hw_run<W, HW_ENDS>(T, ln, plo, phi, text, any_live, sink);
            if (valid && (FILL ? c != room : c == 0)) status = -8;          // a hit has its first end at least; both runs count alike
        }
    }
    if (!FILL && valid) cnt[pair] = status ? 0 : c;
    if (in.flags && __ballot(has && status < -1) != 0 && lane == 0) atomicOr(in.flags, HW_FLAG_STATUS);
}

// The tiles hold entries of the expanded list: in.pt = E.t, in.pk = E.h, he = E.he.  locs[2 i] = smallest start of distance h for the
// entry's end (< -1: internal status -- a true end always has one), locs[2 i + 1] = end.
template <int W>
__global__ __launch_bounds__(256) void k_hw_starts(DevStore S, HwTileIn in, const int32_t *__restrict__ he, int32_t *__restrict__ locs)
{
    const uint32_t slot = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slot >= in.n_tiles) return;
    const uint64_t *planes = S.planes;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(planes);
    const uint32_t nseq = S.n;
    const int32_t nchunks = (int32_t)S.nchunks;
    const uint32_t tile = in.tile_list ? (uint32_t)uniform_i32((int32_t)in.tile_list[slot]) : slot;
    const uint32_t q = (uint32_t)uniform_i32((int32_t)in.tile_q[tile]);
    const int32_t P = uniform_i32(S.lens[q]);
    const uint32_t ent = in.lane_pair[(size_t)tile * 64 + lane];
    const bool has = ent != 0xffffffffu;
    const uint32_t tid = has ? in.pt[ent] : q;
    const int32_t h = has ? he[(size_t)ent * 2] : -1;
    const int32_t end = has ? he[(size_t)ent * 2 + 1] : -1;
    const bool valid = has && h >= 0 && end >= 0 && end < S.lens[tid];
    const int32_t hmax = uniform_i32(wave_max_i32(valid ? h : 0));
    int32_t r_start = has && !valid ? -9 : -1;
    if (2 * hmax + 1 > 64 * W) r_start = valid ? -3 : r_start;
    else if (__ballot(valid) != 0) {
        // ---- START: reversed query against the reversed prefix t[0..end], as in k_hw_finish ----
        auto chunk_lo = [&](int32_t ci) -> uint64_t { return ci >= 0 && ci < nchunks ? planes[((size_t)ci * nseq + q) * 2] : 0; };
        auto chunk_hi = [&](int32_t ci) -> uint64_t { return ci >= 0 && ci < nchunks ? planes[((size_t)ci * nseq + q) * 2 + 1] : 0; };
        auto any_live = [](bool live) { return __ballot(live) != 0; };
        auto nosink = [](int32_t, int, uint64_t, uint64_t) {};
        HwTile T;
        T.P = P; T.a0 = -hmax; T.jx = P - hmax > 1 ? P - hmax : 1;
        HwLane ln;
        const int32_t nc = end + 1 < P + hmax ? end + 1 : P + hmax;
        ln.ncols = valid ? nc : 0; ln.k = h; ln.h = h;
        T.ncols_max = uniform_i32(wave_max_i32(ln.ncols));
        auto plo = [&](int32_t off) { return stream64_rev(chunk_lo, P, off); };
        auto phi = [&](int32_t off) { return stream64_rev(chunk_hi, P, off); };
        auto text = [&](int32_t jb, uint32_t &wl, uint32_t &wh) {       // column c <-> target position end - c
            const int32_t p0 = end - jb - 31;
            wl = __builtin_bitreverse32(hw_text32(pw, nseq, (uint32_t)nchunks, tid, 0, p0));
            wh = __builtin_bitreverse32(hw_text32(pw, nseq, (uint32_t)nchunks, tid, 1, p0));
        };
        hw_run<W, HW_START>(T, ln, plo, phi, text, any_live, nosink);
        if (valid) r_start = ln.r_pl >= 1 ? end - (ln.r_pl - 1) : -4;
    }
    if (has) { locs[(size_t)ent * 2] = r_start; locs[(size_t)ent * 2 + 1] = end; }
    if (in.flags && __ballot(has && r_start < 0) != 0 && lane == 0) atomicOr(in.flags, HW_FLAG_STATUS);
}

}  // namespace isocon
