// hw_rows.hpp -- every best location of the infix ("HW") pairs whose band exceeds the 512 diagonals of hw.hpp: device side of the wide
// part of isocon_hw_locations_wide (the pairs within the band run on hw_loc.hpp).  Two DP runs per pair and no per-column scratch:
//   count run  distance h (or -1 above k), the first end, and how many columns of the query's last row attain h
//   (exclusive scan of the counts -> loc_ptr; its total sizes the output)
//   fill run   the same recurrence with h known: the i-th column attaining h becomes entry loc_ptr[x] + i of the expanded list of
//              hw_loc.hpp (HwLocList: one entry per (pair, end)), never past what the count run found
// by one of two kernels:
//   k_hwl_rows<W, FILL>  one LANE per pair, queries of at most 64 W rows (hw_rows_core.hpp): the query in registers, the target streamed
//                        64 columns per 16-byte load; lanes do not communicate, a wave runs to its longest lane's columns and a finished
//                        lane idles.  No LDS, no scratch.
//   k_hwl_wave<FILL>     one WAVEFRONT per pair, any query: hwf_run<HWF_ENDS> of hw_full.hpp, the lane that owns the query's last row
//                        counts or lists.
// The start of an entry with 2 h + 1 <= 512 comes from k_hw_starts of hw_loc.hpp (band [-h, h] whatever the lengths are: such entries
// carry he[2 i] = h), that of an entry with h > 255 (he[2 i] = -1: the tile builder passes it by) from k_hwl_starts_full, one wavefront
// per entry: the START block of k_hwf_finish without TRACE.
#pragma once
#include "common.hpp"
#include "hw_full.hpp"
#include "hw_loc.hpp"
#include "hw_rows_core.hpp"

namespace isocon {

static constexpr int32_t kHwlBandedStartMax = 255;          // 2 h + 1 <= 512

struct HwlIn {
    const uint32_t *pq, *pt;     // query / target of every wide pair
    const int32_t *pk;           // its threshold
    const uint32_t *list;        // the launch's pairs (indices x into pq / pt / pk)
    uint32_t n;
    int32_t *he;                 // [2 x] = h or -1, [2 x + 1] = first end: written by the count run, read by the fill run
    uint32_t *cnt;               // [x] = ends (count run)
    const unsigned long long *loc_ptr;          // fill run: first entry of pair x, [x + 1] - [x] = what the count run found
    uint32_t *flags;             // bit HW_FLAG_STATUS: the two runs disagree
};

__device__ __forceinline__ void hwl_entry(const HwLocList &E, unsigned long long i, uint32_t q, uint32_t tid, int32_t h, int32_t end)
{
    E.q[i] = q; E.t[i] = tid; E.h[i] = h;
    E.he[i * 2] = h <= kHwlBandedStartMax ? h : -1; E.he[i * 2 + 1] = end;
}

static constexpr uint32_t kHwlRowsBlock = 256;          // (64 measured no faster at 20 000 pairs and 8 % slower at 300 000: DESIGN.md 4.7)

template <int W, int FILL>
__global__ __launch_bounds__(kHwlRowsBlock) void k_hwl_rows(DevStore S, HwlIn in, HwLocList E)
{
    const uint32_t i = blockIdx.x * kHwlRowsBlock + threadIdx.x;
    const bool has = i < in.n;
    const uint32_t x = in.list[has ? i : 0];
    const uint32_t q = in.pq[x], tid = in.pt[x];
    const int32_t k = in.pk[x];
    const int32_t m = S.lens[q], n = S.lens[tid];
    const int32_t h = FILL ? in.he[(size_t)x * 2] : 0;
    const bool valid = has && m > 0 && m <= 64 * W && n > 0 && k >= 0 && n - m >= -k && h >= 0;
    const int32_t ncols = valid ? n : 0;
    const int32_t nmax = uniform_i32(wave_max_i32(ncols));
    const uint64_t *planes = S.planes;
    const uint32_t nseq = S.n;
    const int32_t nchunks = (int32_t)S.nchunks;
    HwrLane<W> L;
    hwr_init<W>(L, [&](int w) -> uint64_t { return valid && w < nchunks ? planes[((size_t)w * nseq + q) * 2] : 0; },
                [&](int w) -> uint64_t { return valid && w < nchunks ? planes[((size_t)w * nseq + q) * 2 + 1] : 0; }, valid ? m : 1);
    const ulonglong2 *P2 = reinterpret_cast<const ulonglong2 *>(planes);
    const unsigned long long base = FILL && valid ? in.loc_ptr[x] : 0;
    const uint32_t room = FILL && valid ? (uint32_t)(in.loc_ptr[x + 1] - base) : 0;
    HwrCount C;
    hwr_count_init(C);
    uint32_t c = 0;
    for (int32_t j0 = 0; j0 < nmax; j0 += 64) {
        ulonglong2 tw = {0, 0};
        if (j0 < ncols) tw = P2[(size_t)(j0 >> 6) * nseq + tid];          // columns <-> target positions, 64 per load
        uint64_t tl = tw.x, th = tw.y;
        const int32_t nb = nmax - j0 < 64 ? nmax - j0 : 64;
        for (int32_t b = 0; b < nb; ++b) {
            const int32_t col = j0 + b;
            if (col < ncols) {
                hwr_step<W>(L, (int32_t)(tl & 1u) | ((int32_t)(th & 1u) << 1));
                if (!FILL) hwr_count_add(C, L.score, col);
                else if (L.score == h) {
                    if (c < room) hwl_entry(E, base + c, q, tid, h, col);
                    ++c;
                }
            }
            tl >>= 1; th >>= 1;
        }
    }
    if (!FILL) {
        if (has) {
            const bool hit = valid && C.best <= k;
            in.he[(size_t)x * 2] = hit ? C.best : -1;
            in.he[(size_t)x * 2 + 1] = hit ? C.first : -1;
            in.cnt[x] = hit ? C.count : 0;
        }
    } else if (valid && c != room) atomicOr(in.flags, HW_FLAG_STATUS);
}

// grid: any number of 64-thread blocks; dynamic LDS: the boundary row of hwf_run when some query has more than one pass
template <int FILL>
__global__ __launch_bounds__(64) void k_hwl_wave(DevStore S, HwlIn in, HwLocList E)
{
    extern __shared__ uint32_t hwf_bound[];
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    for (uint32_t i = blockIdx.x; i < in.n; i += gridDim.x) {
        const uint32_t x = (uint32_t)uniform_i32((int32_t)in.list[i]);
        const uint32_t q = (uint32_t)uniform_i32((int32_t)in.pq[x]), tid = (uint32_t)uniform_i32((int32_t)in.pt[x]);
        const int32_t k = uniform_i32(in.pk[x]);
        const int32_t m = uniform_i32(S.lens[q]), n = uniform_i32(S.lens[tid]);
        const int32_t h = FILL ? uniform_i32(in.he[(size_t)x * 2]) : 0;
        const bool valid = m > 0 && n > 0 && k >= 0 && n - m >= -k && h >= 0;
        const int owner = valid ? ((m - 1) >> 6) & 63 : 0;          // the lane of the query's last row in the last pass
        const unsigned long long base = FILL && valid ? in.loc_ptr[x] : 0;
        const uint32_t room = FILL && valid ? (uint32_t)(in.loc_ptr[x + 1] - base) : 0;
        HwrCount C;
        hwr_count_init(C);
        uint32_t c = 0;
        if (valid) {
            auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {
                wl = hw_text32(pw, S.n, S.nchunks, tid, 0, s);
                wh = hw_text32(pw, S.n, S.nchunks, tid, 1, s);
            };
            auto sink = [&](int32_t score, int32_t col) {
                if (!FILL) hwr_count_add(C, score, col);
                else if (score == h) {
                    if (c < room) hwl_entry(E, base + c, q, tid, h, col);
                    ++c;
                }
            };
            int32_t sc, best, col;
            hwf_run<HWF_ENDS>(S, q, m, n, h, text, hwf_bound, nullptr, false, sc, best, col, sink);
        }
        if ((int)threadIdx.x == owner) {
            if (!FILL) {
                const bool hit = valid && C.best <= k;
                in.he[(size_t)x * 2] = hit ? C.best : -1;
                in.he[(size_t)x * 2 + 1] = hit ? C.first : -1;
                in.cnt[x] = hit ? C.count : 0;
            } else if (valid && c != room) atomicOr(in.flags, HW_FLAG_STATUS);
        }
    }
}

// The entries list[0 .. n) of the expanded list (h > 255): locs[2 i] = smallest start of distance h for the entry's end (< 0: internal
// status, flagged), locs[2 i + 1] = end.  grid: any number of 64-thread blocks; dynamic LDS as k_hwl_wave.
__global__ __launch_bounds__(64) void k_hwl_starts_full(DevStore S, HwLocList E, const uint32_t *__restrict__ list, uint32_t n, int32_t *__restrict__ locs,
                                                         uint32_t *__restrict__ flags)
{
    extern __shared__ uint32_t hwf_bound[];
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(S.planes);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t ent = (uint32_t)uniform_i32((int32_t)list[i]);
        const uint32_t q = (uint32_t)uniform_i32((int32_t)E.q[ent]), tid = (uint32_t)uniform_i32((int32_t)E.t[ent]);
        const int32_t h = uniform_i32(E.h[ent]), end = uniform_i32(E.he[(size_t)ent * 2 + 1]);
        const int32_t m = uniform_i32(S.lens[q]);
        int32_t r_start = -9;
        if (h >= 0 && end >= 0 && end < S.lens[tid] && m > 0) {
            // reversed query against the reversed prefix t[0..end]; a column past m + h cannot hold h
            const int32_t nc = end + 1 < m + h ? end + 1 : m + h;
            auto text = [&](int32_t s, uint32_t &wl, uint32_t &wh) {               // column c <-> target position end - c
                const int32_t p0 = end - s - 31;
                wl = __builtin_bitreverse32(hw_text32(pw, S.n, S.nchunks, tid, 0, p0));
                wh = __builtin_bitreverse32(hw_text32(pw, S.n, S.nchunks, tid, 1, p0));
            };
            int32_t sc, best, col;
            hwf_run<HWF_START>(S, q, m, nc, h, text, hwf_bound, nullptr, false, sc, best, col);
            r_start = col >= 0 ? end - col : -4;
        }
        if (threadIdx.x == 0) {
            locs[(size_t)ent * 2] = r_start; locs[(size_t)ent * 2 + 1] = end;
            if (r_start < 0) atomicOr(flags, HW_FLAG_STATUS);
        }
    }
}

}  // namespace isocon
