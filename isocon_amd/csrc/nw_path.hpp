// nw_path.hpp -- global ("NW") alignment paths for pair lists: device side of edlib.align(q, t, mode="NW", task="path", k)
// (the reference's modules/edlib_alignment_module.py:130-135, edlib_traceback).  Lane-level math, the walk and the op encoding:
// nw_path_core.hpp; the forward pass and the layout of the trace store: hw_full.hpp / hw_full_core.hpp.
//
// The distances are known when these kernels run (isocon_ed_pairs' path, bounded by k; for the infix entry isocon_hw_pairs_wide's,
// with the location): only the pairs within their threshold get here.
//   k_nwp_trace<WINDOW>  one wavefront = one pair.  hwf_run<HWF_TRACE> with every column kept and the top-row delta +1, un-banded,
//                over the WHOLE target (WINDOW = false: start = 0, ms = len t; isocon_ed_path_pairs) or over the located window
//                t[t_start .. t_start + t_cols) alone (WINDOW = true: isocon_hw_path_pairs, the global alignment of the query
//                against that window); its score must equal the known distance.  Then the wave-uniform walk from (m, ms): one
//                request brings 64 columns of the current block -- lane c holds Pv / Ph and the text base of column j - c -- and the
//                block's two query plane words, so telling '=' from 'X' costs no further trip.  Lane 0 writes the runs, REVERSED, into
//                the pair's slice of 2 ed + 1 ops (nwp_max_runs) and the number of runs.
//   k_nwp_emit   one thread = one pair: nwp_forward_runs from that slice to the pair's place in the dense forward list, whose
//                offsets the host made from the run counts.
#pragma once
#include "common.hpp"
#include "hw_full.hpp"
#include "nw_path_core.hpp"

namespace isocon {

struct NwpIn {
    const uint32_t *pq, *pt;     // query / target of the launch's pairs
    const int32_t *ed;           // their distances
    const int32_t *t_start;      // WINDOW only: first target position of every pair's window, and its number of columns; the store
    const int32_t *t_cols;       //              is that of (m, t_cols)
    const uint64_t *trace_off;   // first 16-byte unit of every pair's trace store within the launch's scratch
    const uint64_t *rev_off;     // first op of every pair's slice of the reversed runs
    uint32_t n;
};

// out_runs[x] = number of runs of pair x, or an internal status: -5 the pass' score is not the known distance, -6 more runs than
// 2 ed + 1, -7 (WINDOW) the window is not inside the target.  grid = in.n blocks of 64 threads.
template <bool WINDOW>
__global__ __launch_bounds__(64) void k_nwp_trace(DevStore S, NwpIn in, ulonglong2 *__restrict__ trace_all, uint32_t *__restrict__ rev_all,
                                                   int32_t *__restrict__ out_runs)
{
    extern __shared__ uint32_t nwp_bound[];
    const int lane = threadIdx.x;
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    const uint64_t *planes = S.planes;
    const uint32_t nseq = S.n;
    if (blockIdx.x >= in.n) return;
    const uint32_t x = blockIdx.x;
    const uint32_t q = (uint32_t)uniform_i32((int32_t)in.pq[x]), tid = (uint32_t)uniform_i32((int32_t)in.pt[x]);
    const int32_t m = uniform_i32(S.lens[q]), nt = uniform_i32(S.lens[tid]), ed = uniform_i32(in.ed[x]);
    // the columns of the pass are target positions ts .. ts + n - 1
    const int32_t ts = WINDOW ? uniform_i32(in.t_start[x]) : 0, n = WINDOW ? uniform_i32(in.t_cols[x]) : nt;
    int32_t r = -5;
    if (WINDOW && (ts < 0 || n <= 0 || n > nt - ts)) r = -7;
    else if (m > 0 && n > 0 && ed >= 0) {
        ulonglong2 *trace = trace_all + in.trace_off[x];
        uint32_t *rev = rev_all + in.rev_off[x];
        const int32_t cap = (int32_t)nwp_max_runs(ed);
        auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {
            wl = hw_text32(pw, S.n, S.nchunks, tid, 0, ts + s);
            wh = hw_text32(pw, S.n, S.nchunks, tid, 1, ts + s);
        };
        int32_t sc, best, col;
        hwf_run<HWF_TRACE>(S, q, m, n, ed, text, nwp_bound, trace, true, sc, best, col);
        if (sc == ed) {
            // lane c holds column j0 - c of block b0; qlo / qhi: that block's rows
            int32_t b0 = -1, j0 = 0, cbase = 0;
            uint64_t cpv = 0, cph = 0, qlo = 0, qhi = 0;
            auto load = [&](int32_t b, int32_t j, uint64_t &pv, uint64_t &ph) {
                if (b != b0 || j > j0 || j <= j0 - 64) {
                    b0 = b; j0 = j;
                    const int32_t jj = j - lane;
                    qlo = planes[((size_t)b * nseq + q) * 2]; qhi = planes[((size_t)b * nseq + q) * 2 + 1];
                    if (jj >= 1) {
                        const ulonglong2 u = trace[hwf_trace_unit(m, n, b, jj)];
                        const int32_t p = ts + jj - 1;
                        const uint64_t tl = planes[((size_t)(p >> 6) * nseq + tid) * 2], th = planes[((size_t)(p >> 6) * nseq + tid) * 2 + 1];
                        cpv = u.x; cph = u.y;
                        cbase = (int32_t)((tl >> (p & 63)) & 1) | ((int32_t)((th >> (p & 63)) & 1) << 1);
                    }
                }
                const int src = j0 - j;
                pv = __shfl(cpv, src, 64); ph = __shfl(cph, src, 64);
            };
            auto same_base = [&](int32_t i, int32_t j) -> bool {
                const int32_t bit = (i - 1) & 63;
                const int32_t qb = (int32_t)((qlo >> bit) & 1) | ((int32_t)((qhi >> bit) & 1) << 1);
                return qb == __shfl(cbase, j0 - j, 64);
            };
            int32_t at = 0;
            auto emit = [&](int32_t code, int32_t len) {
                if (at < cap && lane == 0) rev[at] = nwp_op(code, len);
                ++at;
            };
            const int32_t runs = nwp_walk(m, n, load, same_base, emit);
            r = runs <= cap ? runs : -6;
        }
    }
    if (lane == 0) out_runs[x] = r;
}

// fwd_off[x]: first op of pair x in the dense forward list.  grid: (n + 255) / 256 blocks of 256 threads.
__global__ __launch_bounds__(256) void k_nwp_emit(const uint32_t *__restrict__ rev_all, const uint64_t *__restrict__ rev_off, const int32_t *__restrict__ runs,
                                                   const uint64_t *__restrict__ fwd_off, uint32_t n, uint32_t *__restrict__ fwd_all)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n || runs[x] <= 0) return;
    (void)nwp_forward_runs(rev_all + rev_off[x], (uint64_t)runs[x], fwd_all + fwd_off[x]);
}

}  // namespace isocon
