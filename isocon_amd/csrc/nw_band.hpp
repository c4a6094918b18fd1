// nw_band.hpp -- global ("NW") alignment paths for pair lists, BANDED: the paths of nw_path.hpp for the hits whose corridor -- the
// diagonals an optimal path of the known distance can touch, at most ed + 1 -- fits a window of 64 W rows, W = 1, 2 or 4 (the hit's CLASS).
// Lane-level math, the window placement, the masked walk: nw_band_core.hpp.
//
//   k_nwb_trace<W, WINDOW>   one LANE = one pair, with its own query and its own target (WINDOW = false: the whole target,
//                isocon_ed_path_pairs) or located window of it (WINDOW = true: isocon_hw_path_pairs; the text is read unaligned as
//                hw_text32 reads it).  The forward pass keeps 16 bytes (vertical / horizontal +1 vector) per column and window word
//                instead of per column and 64-row block of the whole query.  The trace store of a wave is laid out [column][word][lane]:
//                what the wave stores for one column is one contiguous run of 64 W 16 bytes; its region holds the columns of its
//                longest lane, so the host puts hits of similar length into a wave.  Text and query words of the next block of 32 columns
//                are requested before the current block's columns are computed.  Then every lane walks its own path from (m, n): the
//                units of the 8 columns ahead of the walk are fetched together and kept in LDS, the plane words of the two sequences
//                stay in registers for 64 positions.  The lane writes its runs, REVERSED, into its slice of 2 ed + 1 ops and its number
//                of runs, in the format of k_nwp_trace, so that k_nwp_emit serves both.
#pragma once
#include "common.hpp"
#include "hw.hpp"
#include "nw_band_core.hpp"
#include "nw_path.hpp"

namespace isocon {

static constexpr int NWB_CACHE = 8;          // columns the walk fetches at a time

struct NwbIn {
    const uint32_t *slot_hit;    // [waves][64]: the hit of every lane of the launch's waves, 0xffffffff = none
    const uint64_t *wave_off;    // first 16-byte unit of every wave's region within the launch's scratch
    const int32_t *wave_cols;    // columns that region holds, and
    const int32_t *wave_lanes;   // its lanes (the stride between its words): 64, less for the last wave of a class or one cut down to the budget
    const uint32_t *pq, *pt;     // by hit: query / target,
    const int32_t *ed;           //         distance,
    const int32_t *t_start;      //         WINDOW only: first target position of the window and its number of columns,
    const int32_t *t_cols;
    const uint64_t *rev_off;     //         first op of the slice of the reversed runs
    uint32_t n_waves;
};

// out_runs[hit] = number of runs, or an internal status: -5 the pass' score is not the known distance (or the hit is not of this class, or
// its columns exceed the wave's region), -6 more runs than 2 ed + 1, -7 (WINDOW) the window is not inside the target.
// grid = in.n_waves blocks of 64 threads.
template <int W, bool WINDOW>
__global__ __launch_bounds__(64) void k_nwb_trace(DevStore S, NwbIn in, ulonglong2 *__restrict__ trace_all, uint32_t *__restrict__ rev_all,
                                                   int32_t *__restrict__ out_runs)
{
    __shared__ ulonglong2 nwb_cache[NWB_CACHE][64];
    const int lane = threadIdx.x;
    if (blockIdx.x >= in.n_waves) return;
    const uint32_t wave = blockIdx.x;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    const uint64_t *planes = S.planes;
    const uint32_t nseq = S.n;
    const int32_t wcols = uniform_i32(in.wave_cols[wave]), nl = uniform_i32(in.wave_lanes[wave]);
    const uint32_t hit = in.slot_hit[(size_t)wave * 64 + lane];
    const bool has = hit != 0xffffffffu && lane < nl;
    uint32_t q = 0, tid = 0;
    int32_t m = 0, n = 0, nt = 0, ts = 0, ed = 0;
    if (has) {
        q = in.pq[hit]; tid = in.pt[hit]; ed = in.ed[hit];
        if (q >= nseq || tid >= nseq) { q = 0; tid = 0; ed = -1; }
        m = S.lens[q]; nt = S.lens[tid];
        ts = WINDOW ? in.t_start[hit] : 0;
        n = WINDOW ? in.t_cols[hit] : nt;
    }
    int32_t r = -5, a0 = 0;
    bool run = false;
    if (has) {
        if (WINDOW && (ts < 0 || n <= 0 || n > nt - ts)) { r = -7; ts = 0; n = 0; }
        else if (m > 0 && n > 0 && n <= wcols && ed >= 0) {
            const int32_t cls = nwb_class(m - n, ed);
            if (cls >= 1 && cls <= W) { run = true; a0 = nwb_origin(m - n, ed, W); }
        }
    }
    // this lane's unit of column col (0-based) and window word w
    ulonglong2 *trace = trace_all + in.wave_off[wave] + lane;
    const size_t stride = (size_t)nl;
    auto qw = [&](int plane, int32_t p) -> uint32_t { return hw_text32(pw, nseq, S.nchunks, q, plane, p); };
    auto tw = [&](int plane, int32_t p) -> uint32_t { return hw_text32(pw, nseq, S.nchunks, tid, plane, ts + p); };
    // (a lane that has finished, or has no pair, goes through a full block with the others: the columns it hands over are below those of
    // a running lane, hence inside the region; a lane outside the region's lanes stores nothing)
    auto sink = [&](int32_t col, int w, uint64_t vp, uint64_t hp) {
        if (has) trace[((size_t)col * W + (size_t)w) * stride] = make_ulonglong2(vp, hp);
    };
    const bool pass = run;
    const int32_t sc = nwb_forward<W>(qw, tw, m, n, a0, run, sink, [](bool b) { return __ballot(b) != 0; });
    if (pass && sc == ed) {
        uint32_t *rev = rev_all + in.rev_off[hit];
        const int32_t cap = (int32_t)nwp_max_runs(ed);
        // the cache holds the units of word wc of the columns jc, jc - 1, .. jc - NWB_CACHE + 1
        // and ql .. th the plane bits of the query positions qb0 .. qb0 + 63 and of the target positions tb0 .. tb0 + 63.  A lane moves
        // at most one column and one position per step, and the lanes that still walk are at this point together: when one of them runs
        // out, ALL fetch again from where they stand, so that the wave waits for memory once per 8 steps (units) and once per 64 (planes)
        // instead of once per step for one lane or another.
        int32_t jc = 0, wc = -1, qb0 = -(1 << 30), tb0 = -(1 << 30);
        uint64_t ql = 0, qh = 0, tl = 0, th = 0;
        const int32_t nchunks = (int32_t)S.nchunks;
        auto load = [&](int32_t i, int32_t j, int32_t w, uint64_t &vp, uint64_t &hp) {
            if (__ballot(w != wc || j > jc || j <= jc - NWB_CACHE) != 0) {
                wc = w; jc = j;
#pragma unroll
                for (int t = 0; t < NWB_CACHE; ++t)
                    if (j - t >= 1) nwb_cache[t][lane] = trace[((size_t)(j - t - 1) * W + (size_t)w) * stride];
            }
            const int32_t qi = i - 1, tp = ts + j - 1;
            if (__ballot(qi < qb0 || qi > qb0 + 63 || tp < tb0 || tp > tb0 + 63) != 0) {
                qb0 = qi - 63; tb0 = tp - 63;
                ql = stream64([&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + q) * 2] : 0; }, qb0);
                qh = stream64([&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + q) * 2 + 1] : 0; }, qb0);
                tl = stream64([&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + tid) * 2] : 0; }, tb0);
                th = stream64([&](int32_t ci) -> uint64_t { return ci < nchunks ? planes[((size_t)ci * nseq + tid) * 2 + 1] : 0; }, tb0);
            }
            const ulonglong2 u = nwb_cache[jc - j][lane];
            vp = u.x; hp = u.y;
        };
        auto side = [&](int32_t j, int32_t w, uint64_t &vp, uint64_t &hp) {
            const ulonglong2 u = trace[((size_t)(j - 1) * W + (size_t)w) * stride];
            vp = u.x; hp = u.y;
        };
        auto same_base = [&](int32_t i, int32_t j) -> bool {
            const int32_t qs = i - 1 - qb0, tsh = ts + j - 1 - tb0;          // 0 .. 63: the last load made sure
            return ((((ql >> qs) ^ (tl >> tsh)) | ((qh >> qs) ^ (th >> tsh))) & 1) == 0;
        };
        int32_t at = 0;
        auto emit = [&](int32_t code, int32_t len) {
            if (at < cap) rev[at] = nwp_op(code, len);
            ++at;
        };
        const int32_t runs = nwb_walk<W>(m, n, a0, load, side, same_base, emit);
        r = runs < 0 ? runs : runs <= cap ? runs : -6;
    }
    if (has) out_runs[hit] = r;
}

}  // namespace isocon
