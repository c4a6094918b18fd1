// shw.hpp -- prefix ("SHW") alignments of a pair list: device side of isocon_shw_locations and isocon_shw_path_pairs, what
// edlib.align(q, t, mode="SHW", k) answers -- the whole query against a PREFIX of the target (a primer that must sit at the read's start;
// on reversed strings the read's end).  With D the global matrix (row 0 = j, column 0 = i): h = min over columns j >= 1 of D[P][j], the
// ends every 0-based column j - 1 with D[P][j] == h; the start is 0.  Lane-level math: hw_core.hpp (modes PREFIX_LOCATE and PREFIX_ENDS);
// tiles as in hw.hpp: one wavefront = one shared query (rows, wave-uniform window) x up to 64 lane targets (columns) -- one primer
// against 64 reads.  The band is [-kmax, kmax] whatever the targets' lengths are: only the first P + k columns of a target matter.
//   k_shw_round        the threshold of every pair in round r of the distance stage (thresholds 31, 63, 127, 255 capped by the pair's
//                      own: the classes of 1, 2, 4, 8 words), HWT_SKIP for a settled pair; counts the pairs that enter the round
//   k_shw_locate<W>    PREFIX_LOCATE: (h or -1, first end) per pair of the round's tiles
//   k_shw_prep         thr[p] = h or HWT_SKIP -- the threshold of the ENDS tiles --, cnt[p] = 0
//   k_shw_ends<W, 0>   PREFIX_ENDS on the hits, tiles built with threshold h: cnt[p] = ends of pair p (at most 2 h + 1)
//   (exclusive scan of cnt -> end_ptr; its total sizes the output)
//   k_shw_ends<W, 1>   the same run again: end i of pair p written to ends[end_ptr[p] + i]
#pragma once
#include "common.hpp"
#include "hw.hpp"
#include "hw_tiles.hpp"

namespace isocon {

// thresholds of the rounds: 32 * 2^r - 1, i.e. 2 thr + 1 = 63, 127, 255, 511 diagonals
__host__ __device__ __forceinline__ int32_t shw_round_thr(int r) { return (32 << r) - 1; }
static constexpr int SHW_ROUNDS = 4;

// Round r: thr[p] = min(kc, shw_round_thr(r)) for a pair that is not settled yet, kc = min(k[p], len(q)) (h <= len(q): a larger threshold
// asks nothing more); HWT_SKIP for one that is -- it hit in an earlier round, or missed at its own threshold.  A pair whose arguments the
// tile builder will refuse (id out of range, k < 0) is handed on as it is.  Round 0 also writes the "no hit" rows of he.
// entering[r] += pairs that take part in the round.
__global__ __launch_bounds__(256) void k_shw_round(DevStore S, const uint32_t *__restrict__ q, const uint32_t *__restrict__ t, const int32_t *__restrict__ k,
                                                    unsigned long long n_pairs, int r, int32_t *__restrict__ he, int32_t *__restrict__ thr,
                                                    uint32_t *__restrict__ entering)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    bool in = false;
    if (p < n_pairs) {
        const uint32_t qq = q[p], tt = t[p];
        const int32_t kv = k[p];
        int32_t out = kv < 0 ? -1 : kv;          // (k < 0: the builder flags it, whatever its value)
        if (r == 0) { he[p * 2] = -1; he[p * 2 + 1] = -1; }
        if (qq < S.n && tt < S.n && kv >= 0) {
            const int32_t lq = S.lens[qq];
            const int32_t kc = kv < lq ? kv : lq;
            const bool open = r == 0 || (he[p * 2] == -1 && shw_round_thr(r - 1) < kc);
            const int32_t tr = shw_round_thr(r);
            out = open ? (kc < tr ? kc : tr) : HWT_SKIP;
            in = open;
        } else if (r > 0) out = HWT_SKIP;          // (round 0 has refused the call)
        thr[p] = out;
    }
    const uint64_t m = __ballot(in);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(entering + r, (uint32_t)__builtin_popcountll(m));
}

__global__ __launch_bounds__(256) void k_shw_prep(const int32_t *__restrict__ he, unsigned long long n_pairs, int32_t *__restrict__ thr, uint32_t *__restrict__ cnt)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t h = he[p * 2];
    thr[p] = h >= 0 ? h : HWT_SKIP;
    cnt[p] = 0;
}

// the geometry both kernels share: wave-uniform tile and this lane's columns.  false: the tile has no valid lane.
struct ShwGeom {
    HwTile T;
    int32_t ncols;       // this lane's columns (0: not valid)
    int32_t rows;        // diagonals of the tile's band
};

__device__ __forceinline__ bool shw_geom(int32_t P, int32_t n, int32_t thr, bool has, ShwGeom &G, bool &valid)
{
    valid = has && P > 0 && n > 0 && thr >= 0 && n - P >= -thr;
    const int32_t kmax = uniform_i32(wave_max_i32(valid ? thr : -1));
    if (kmax < 0) return false;
    const int32_t nc = n < P + thr ? n : P + thr;
    G.ncols = valid ? nc : 0;
    G.rows = 2 * kmax + 1;
    G.T.P = P; G.T.a0 = -kmax; G.T.jx = P - kmax > 1 ? P - kmax : 1;
    G.T.ncols_max = uniform_i32(wave_max_i32(G.ncols));
    return true;
}

// in.pk = the round's thresholds (k_shw_round).  out_he[2 p] = distance (-1: above the threshold, -3: the tile's band does not fit W
// words), out_he[2 p + 1] = first end.  Launch shape of k_hw_locate: 256 threads, four tiles per workgroup.
template <int W>
__global__ __launch_bounds__(256) void k_shw_locate(DevStore S, HwTileIn in, int32_t *__restrict__ out_he)
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
    const int32_t k = has ? in.pk[pair] : -1;
    const int32_t m = S.lens[tid];
    ShwGeom G;
    bool valid;
    int32_t r_h = -1, r_end = -1;
    if (shw_geom(P, m, k, has, G, valid)) {
        if (G.rows > 64 * W) r_h = -3;
        else {
            HwLane ln;
            ln.ncols = G.ncols; ln.k = k; ln.h = 0;
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
                if ((jb & 63) == 0) tcur = (jb >> 6) < nchunks ? P2[(size_t)(jb >> 6) * nseq + tid] : ulonglong2{0, 0};       // columns <-> target positions, 64 per load
                wl = (uint32_t)((jb & 32) ? (tcur.x >> 32) : tcur.x);
                wh = (uint32_t)((jb & 32) ? (tcur.y >> 32) : tcur.y);
            };
            auto any_live = [](bool live) { return __ballot(live) != 0; };
            auto nosink = [](int32_t, int, uint64_t, uint64_t) {};
            hw_run<W, HW_PREFIX_LOCATE>(G.T, ln, plo, phi, text, any_live, nosink);
            if (valid && ln.r_h <= k) { r_h = ln.r_h; r_end = ln.r_end; }
        }
    }
    if (has) { out_he[(size_t)pair * 2] = r_h; out_he[(size_t)pair * 2 + 1] = r_end; }
    if (in.flags && __ballot(has && r_h < -1) != 0 && lane == 0) atomicOr(in.flags, HW_FLAG_STATUS);
}

// in.pk = thr (k_shw_prep): the tiles hold hits only.  FILL = 0: cnt[pair] = ends; FILL = 1: ends[end_ptr[pair] ..], ascending.
template <int W, int FILL>
__global__ __launch_bounds__(256) void k_shw_ends(DevStore S, HwTileIn in, uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ end_ptr,
                                                   int32_t *__restrict__ ends)
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
    ShwGeom G;
    bool valid;
    int32_t status = 0;
    uint32_t c = 0;
    if (shw_geom(P, m, h, has, G, valid)) {
        if (G.rows > 64 * W) status = -3;
        else {
            HwLane ln;
            ln.ncols = G.ncols; ln.k = h; ln.h = h;
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
                if ((jb & 63) == 0) tcur = (jb >> 6) < nchunks ? P2[(size_t)(jb >> 6) * nseq + tid] : ulonglong2{0, 0};
                wl = (uint32_t)((jb & 32) ? (tcur.x >> 32) : tcur.x);
                wh = (uint32_t)((jb & 32) ? (tcur.y >> 32) : tcur.y);
            };
            auto any_live = [](bool live) { return __ballot(live) != 0; };
            const unsigned long long base = FILL && valid ? end_ptr[pair] : 0;
            const unsigned long long room = FILL && valid ? end_ptr[pair + 1] - base : 0;          // (what the count run found: never written past)
            auto sink = [&](int32_t end, int, uint64_t, uint64_t) {
                if (FILL && c < room) ends[base + c] = end;
                ++c;
            };
            hw_run<W, HW_PREFIX_ENDS>(G.T, ln, plo, phi, text, any_live, sink);
            if (valid && (FILL ? c != room : c == 0)) status = -8;          // a hit has its first end at least; both runs count alike
        }
    }
    if (!FILL && valid) cnt[pair] = status ? 0 : c;
    if (in.flags && __ballot(has && status < -1) != 0 && lane == 0) atomicOr(in.flags, HW_FLAG_STATUS);
}

}  // namespace isocon
