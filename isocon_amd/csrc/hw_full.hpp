// hw_full.hpp -- un-banded infix ("HW") alignment for the pairs whose band exceeds the 512 diagonals of hw.hpp: device side of
// edlib.align(q, t, mode="HW", task="path", k) for ANY k (/root/reference/modules/end_invariant_functions.py:593-620 edlib_traceback
// with a large k, :622-681 get_all_NN with a large ignore_ends_len).  Lane-level math, the three passes and the layout of the trace
// store: hw_full_core.hpp.
//
// One wavefront = one pair.  Lane l owns query rows 64 l .. 64 l + 63 of the current pass, the column loop is systolic (lane l works
// on column s - l at step s; the base and the horizontal delta go one lane down per step in one shuffle), queries above 4 096 rows
// run in passes of 64 blocks whose boundary row goes through a 2-bit-per-column buffer in LDS.
//   k_hwf_locate  pass LOCATE                              -> (h or -1, end) per pair
//   k_hwf_finish  passes START and TRACE + the walk, hits  -> start, leading / trailing insertion run
// HBM traffic of a hit: 8 bytes per block for the last column, and -- only when start == 0, the one case that can have a leading
// insertion run -- 16 bytes per block and column of stored Pv / Ph, written as runs of 16 x lanes bytes per step (1 KB for a full
// pass), read back once by the walk, 64 columns of one block per request.
#pragma once
#include "common.hpp"
#include "hw.hpp"
#include "hw_full_core.hpp"

namespace isocon {

struct HwfIn {
    const uint32_t *pq, *pt;     // query / target of every wide pair
    const int32_t *pk;           // its threshold
    const uint32_t *list;        // k_hwf_finish: the launch's pairs (indices into pq / pt / pk); k_hwf_locate takes 0 .. n - 1
    const uint64_t *trace_off;   // k_hwf_finish: first 16-byte unit of every listed pair's trace store
    uint32_t n;
};

// All passes of one mode for the wavefront's pair.  text(s, wl, wh): the 32 text bits of columns s .. s + 31 (s a multiple of 32,
// wave-uniform).  bound: LDS, hwf_bound_words(ncols) words when the query has more than one pass.  TRACE: store = the pair's trace
// store, whose head takes the last column; keep_cols: every column is kept as well.  The results are those of the query's last row,
// the same in every lane.  ENDS: sink(score, col) after every column of the query's last row, in the lane that owns that row.
struct HwfNoSink { __device__ __forceinline__ void operator()(int32_t, int32_t) const {} };
template <int MODE, class Text, class Sink = HwfNoSink>
__device__ __forceinline__ void hwf_run(const DevStore &S, uint32_t q, int32_t m, int32_t ncols, int32_t h, Text text, uint32_t *bound,
                                        ulonglong2 *store, bool keep_cols, int32_t &r_score, int32_t &r_best, int32_t &r_col, Sink sink = Sink())
{
    const int lane = threadIdx.x;
    const uint64_t *planes = S.planes;
    const uint32_t nseq = S.n;
    const int32_t nchunks = (int32_t)S.nchunks;
    auto chunk_lo = [&](int32_t ci) -> uint64_t { return ci >= 0 && ci < nchunks ? planes[((size_t)ci * nseq + q) * 2] : 0; };
    auto chunk_hi = [&](int32_t ci) -> uint64_t { return ci >= 0 && ci < nchunks ? planes[((size_t)ci * nseq + q) * 2 + 1] : 0; };
    const int32_t passes = hwf_passes(m);
    uint64_t *fin = reinterpret_cast<uint64_t *>(store);
    r_score = HWB_INF; r_best = HWB_INF; r_col = -1;
    for (int32_t pass = 0; pass < passes; ++pass) {
        const int32_t nbl = hwf_pass_lanes(m, pass);
        const int32_t blk = pass * 64 + lane, row0 = blk * 64;
        HwfLane L;
        if (MODE == HWF_START) hwf_lane_init(L, stream64_rev(chunk_lo, m, row0), stream64_rev(chunk_hi, m, row0), m, row0);
        else hwf_lane_init(L, chunk_lo(blk), chunk_hi(blk), m, row0);
        ulonglong2 *tp = MODE == HWF_TRACE && keep_cols ? store + hwf_pass_base(m, ncols, pass) : nullptr;
        int32_t packed = hwf_pack(0, 0);
        uint32_t bw = 0, wl = 0, wh = 0;
        const int32_t steps = ncols + nbl - 1;
        for (int32_t s = 0; s < steps; ++s) {
            if ((s & 31) == 0) text(s, wl, wh);
            const int32_t recv = __shfl_up(packed, 1, 64);
            int32_t ch, hin;
            if (lane == 0) {
                ch = (int32_t)(((wl >> (s & 31)) & 1u) | (((wh >> (s & 31)) & 1u) << 1));
                hin = pass == 0 ? (MODE == HWF_LOCATE || MODE == HWF_ENDS ? 0 : 1) : (s < ncols ? hwf_bound_get(bound[s >> 4], s) : 0);
            } else {
                ch = hwf_packed_base(recv);
                hin = hwf_packed_delta(recv);
            }
            const int32_t col = s - lane;
            int32_t hout = 0;
            if (col >= 0 && col < ncols && lane < nbl) {
                uint64_t ph;
                hout = hwf_step<MODE>(L, ch, hin, col, h, ph);
                if (MODE == HWF_TRACE) {
                    if (tp) tp[(size_t)s * nbl + lane] = make_ulonglong2(L.Pv, ph);
                    if (col == ncols - 1 && fin) fin[blk] = L.Pv;
                }
                if (MODE == HWF_ENDS && blk == ((m - 1) >> 6)) sink(L.score, col);
                if (lane == 63 && pass + 1 < passes) {
                    bw = hwf_bound_add(bw, col, hout);
                    if (hwf_bound_full(col, ncols)) { bound[col >> 4] = bw; bw = 0; }
                }
            }
            packed = hwf_pack(ch, hout);
        }
        if (pass == passes - 1) {
            const int32_t lstar = ((m - 1) >> 6) - pass * 64;
            r_score = __shfl(L.score, lstar, 64); r_best = __shfl(L.best, lstar, 64); r_col = __shfl(L.best_col, lstar, 64);
        }
        __syncthreads();          // the boundary row (LDS) and the stored columns (memory) are another lane's to read
    }
}

// out_he[2 x] = distance (-1: above k), out_he[2 x + 1] = end, x = index of the pair in the wide list.  grid: any number of 64-thread blocks.
__global__ __launch_bounds__(64) void k_hwf_locate(DevStore S, HwfIn in, int32_t *__restrict__ out_he)
{
    extern __shared__ uint32_t hwf_bound[];
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    for (uint32_t x = blockIdx.x; x < in.n; x += gridDim.x) {
        const uint32_t q = (uint32_t)uniform_i32((int32_t)in.pq[x]), tid = (uint32_t)uniform_i32((int32_t)in.pt[x]);
        const int32_t k = uniform_i32(in.pk[x]);
        const int32_t m = uniform_i32(S.lens[q]), n = uniform_i32(S.lens[tid]);
        int32_t r_h = -1, r_end = -1;
        if (m > 0 && n > 0 && k >= 0 && n - m >= -k) {
            auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {
                wl = hw_text32(pw, S.n, S.nchunks, tid, 0, s);
                wh = hw_text32(pw, S.n, S.nchunks, tid, 1, s);
            };
            int32_t sc, best, col;
            hwf_run<HWF_LOCATE>(S, q, m, n, 0, text, hwf_bound, nullptr, false, sc, best, col);
            if (best <= k) { r_h = best; r_end = col; }
        }
        if (threadIdx.x == 0) { out_he[(size_t)x * 2] = r_h; out_he[(size_t)x * 2 + 1] = r_end; }
    }
}

// Hits only (he[2 x] = h >= 0, he[2 x + 1] = end).  out[5 x ..] = h, start, end, leading / trailing insertion run (h < -1: internal
// status).  grid = in.n blocks of 64 threads, block b works on pair in.list[b] with the store trace + in.trace_off[b].
__global__ __launch_bounds__(64) void k_hwf_finish(DevStore S, HwfIn in, const int32_t *__restrict__ he, ulonglong2 *__restrict__ trace_all,
                                                    int32_t *__restrict__ out)
{
    extern __shared__ uint32_t hwf_bound[];
    const int lane = threadIdx.x;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    if (blockIdx.x >= in.n) return;
    const uint32_t x = (uint32_t)uniform_i32((int32_t)in.list[blockIdx.x]);
    const uint32_t q = (uint32_t)uniform_i32((int32_t)in.pq[x]), tid = (uint32_t)uniform_i32((int32_t)in.pt[x]);
    const int32_t m = uniform_i32(S.lens[q]);
    const int32_t h = uniform_i32(he[(size_t)x * 2]), end = uniform_i32(he[(size_t)x * 2 + 1]);
    ulonglong2 *trace = trace_all + in.trace_off[blockIdx.x];
    int32_t r0 = h, r_start = -1, r_lead = 0, r_trail = 0;
    if (h >= 0 && end >= 0 && m > 0) {
        int32_t sc, best, col;
        // ---- START: reversed query against the reversed prefix t[0..end]; a column past m + h cannot hold h ----
        {
            const int32_t nc = end + 1 < m + h ? end + 1 : m + h;
            auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {               // column c <-> target position end - c
                const int32_t p0 = end - s - 31;
                wl = __builtin_bitreverse32(hw_text32(pw, S.n, S.nchunks, tid, 0, p0));
                wh = __builtin_bitreverse32(hw_text32(pw, S.n, S.nchunks, tid, 1, p0));
            };
            hwf_run<HWF_START>(S, q, m, nc, h, text, hwf_bound, nullptr, false, sc, best, col);
        }
        if (col < 0) r0 = -4;
        else {
            const int32_t start = end - col, ms = col + 1;
            // ---- TRACE: query against t[start..end].  A path that begins with a query-only step could trade it for a diagonal step
            // into t[start - 1] at no cost, so with the SMALLEST start only start == 0 can have a leading run (hw.hpp): the other
            // pairs keep the last column alone. ----
            auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {
                wl = hw_text32(pw, S.n, S.nchunks, tid, 0, start + s);
                wh = hw_text32(pw, S.n, S.nchunks, tid, 1, start + s);
            };
            const uint64_t *fin = reinterpret_cast<const uint64_t *>(trace);
            hwf_run<HWF_TRACE>(S, q, m, ms, h, text, hwf_bound, trace, start == 0, sc, best, col);
            if (sc != h) r0 = -5;
            else {
                r_start = start;
                r_trail = hwf_trail(m, [&](int32_t b) -> uint64_t { return fin[b]; });
                if (start == 0) {
                    // the walk is wave-uniform: lane c holds column j0 - c of block b0, a request serves 64 columns of one block
                    int32_t b0 = -1, j0 = 0;
                    uint64_t cpv = 0, cph = 0;
                    r_lead = hwf_walk(m, ms, [&](int32_t b, int32_t j, uint64_t &pv, uint64_t &ph) {
                        if (b != b0 || j > j0 || j <= j0 - 64) {
                            b0 = b; j0 = j;
                            const int32_t jj = j - lane;
                            if (jj >= 1) { const ulonglong2 u = trace[hwf_trace_unit(m, ms, b, jj)]; cpv = u.x; cph = u.y; }
                        }
                        const int src = j0 - j;
                        pv = __shfl(cpv, src, 64); ph = __shfl(cph, src, 64);
                    });
                }
            }
        }
    }
    if (lane == 0) {
        int32_t *o = out + (size_t)x * 5;
        const bool fine = r0 >= 0;
        o[0] = r0; o[1] = fine ? r_start : -1; o[2] = fine ? end : -1; o[3] = fine ? r_lead : 0; o[4] = fine ? r_trail : 0;
    }
}

}  // namespace isocon
