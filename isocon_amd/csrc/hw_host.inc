// hw_host.inc -- host side of isocon_hw_pairs (included by isocon_hip.hip): tiles of one query x up to 64 targets for the
// bit-parallel kernels of hw.hpp.

namespace {

inline int hw_words(int32_t rows) { return rows <= 64 ? 1 : rows <= 128 ? 2 : rows <= 256 ? 4 : rows <= 512 ? 8 : 0; }

// isocon_hw_last_stats: the calling thread's last isocon_hw_pairs call (and what hw_pairs_device_core did for the entries that share it).
// HS_LOCATE / HS_FINISH / HS_GRID + c: class c = 0 .. 3 (1, 2, 4, 8 window words).  -1: not counted on that route.
enum { HS_ROUTE = 0, HS_RETRIED_HOST, HS_PAIRS, HS_NEED_KERNEL, HS_HITS, HS_LOCATE, HS_FINISH = HS_LOCATE + 4, HS_GRID = HS_FINISH + 4, HS_COUNT = HS_GRID + 4 };
thread_local double g_hw_stats[HS_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline void hw_stats_route(int route, uint64_t n_pairs)
{
    for (int i = 0; i < HS_COUNT; ++i) if (route == 1 || i != HS_RETRIED_HOST) g_hw_stats[i] = 0;          // (the host route may be the retry)
    g_hw_stats[HS_ROUTE] = route;
    g_hw_stats[HS_PAIRS] = (double)n_pairs;
}

// Tiles of the pairs `idx` (any order): pairs are grouped by (words needed, query) with two counting sorts, a group is cut
// into tiles of at most 64 lanes whose COMMON window (largest length difference and largest threshold of the tile) still
// fits the class.  rows(p) = rows of the band pair p needs on its own; fits(dmax, kmax, W) = do these extremes fit W words.
struct HwTiles {
    std::vector<uint32_t> tile_q[4], lane_pair[4];      // per class W = 1, 2, 4, 8
};

template <class Words, class Fits>
void hw_build_tiles(const std::vector<uint32_t> &idx, const uint32_t *q, uint32_t nseq, Words words_of, Fits fits, HwTiles &out)
{
    // stable counting sort by query, then a stable split by class
    std::vector<uint32_t> first((size_t)nseq + 1, 0);
    for (uint32_t p : idx) ++first[(size_t)q[p] + 1];
    for (uint32_t i = 0; i < nseq; ++i) first[i + 1] += first[i];
    std::vector<uint32_t> byq(idx.size());
    for (uint32_t p : idx) byq[first[q[p]]++] = p;
    static const int cls_of[9] = {-1, 0, 1, -1, 2, -1, -1, -1, 3};
    for (int c = 0; c < 4; ++c) {
        const int Wc = 1 << c;
        std::vector<uint32_t> &tq = out.tile_q[c], &lp = out.lane_pair[c];
        uint32_t cur_q = 0xffffffffu;
        int32_t dmax = 0, kmax = 0;
        size_t fill = 64;
        for (uint32_t p : byq) {
            if (cls_of[words_of(p)] != c) continue;
            int32_t d2 = dmax, k2 = kmax;
            const bool same = q[p] == cur_q && fill < 64 && fits(p, d2, k2, Wc);
            if (!same) {
                while (fill < 64 && !tq.empty()) { lp.push_back(0xffffffffu); ++fill; }
                tq.push_back(q[p]);
                cur_q = q[p];
                fill = 0;
                d2 = -(1 << 30); k2 = 0;
                fits(p, d2, k2, Wc);
            }
            dmax = d2; kmax = k2;
            lp.push_back(p);
            ++fill;
        }
        while (fill < 64 && !tq.empty()) { lp.push_back(0xffffffffu); ++fill; }
    }
}

template <int W>
int hw_launch_locate(isocon_store *st, const HwTileIn &in, int32_t *d_he)
{
    hipLaunchKernelGGL((k_hw_locate<W>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_he);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

// k_hw_finish<1|2> keeps checkpoints of the band state (every HW_SEG-th column) in its per-workgroup store and walks on segments
// recomputed into LDS; the wider classes store every column.
inline size_t hw_finish_lds(int Wc) { return Wc == 2 ? (size_t)HW_SEG * 2 * Wc * 64 * 8 : 0; }          // (one word: the segment stays in registers)
inline uint64_t hw_finish_store_bytes(int Wc, uint32_t trace_cols)
{
    return Wc <= 2 ? ((uint64_t)trace_cols / HW_SEG + 2) * 2 * Wc * 64 * 8 : ((uint64_t)trace_cols + 1) * 2 * Wc * 64 * 8;
}
inline uint32_t hw_finish_grid_cap(int Wc) { return Wc == 2 ? (uint32_t)(256 * (160 * 1024 / (hw_finish_lds(Wc) + 256))) : 4096u; }

template <int W>
int hw_launch_finish(isocon_store *st, const HwTileIn &in, uint32_t grid, const int32_t *d_he, uint64_t *d_trace, uint32_t trace_cols, int32_t *d_out)
{
    hipLaunchKernelGGL((k_hw_finish<W>), dim3(grid), dim3(64), hw_finish_lds(W), 0, st->dev, in, d_he, d_trace, trace_cols, d_out);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

}  // namespace

namespace {

// Tiles built on the host (two counting sorts and a greedy cut, hw_build_tiles): small calls, and calls where a run of 64 pairs of one
// query has a common window wider than 512 diagonals although every pair fits on its own.
int hw_pairs_host_tiles(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out, float *kernel_ms)
{
    const uint32_t n = s->dev.n;
    const std::vector<int32_t> &lens = s->lens;
    hw_stats_route(0, n_pairs);
    // pairs that need no kernel (distance >= len(q) - len(t) > k, or an empty sequence) and the band every other pair needs
    std::vector<uint32_t> run;
    run.reserve(n_pairs);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (q[p] >= n || t[p] >= n) return ISOCON_E_ARG;
        const int32_t kk = k[p];
        if (kk < 0) { g_last_error = "isocon_hw_pairs: k must be >= 0 (the band is derived from it)"; return ISOCON_E_ARG; }
        if (kk > (1 << 20)) return ISOCON_E_UNSUPPORTED;
        int32_t *o = out + p * 5;
        o[0] = -1; o[1] = -1; o[2] = -1; o[3] = 0; o[4] = 0;
        const int32_t delta = lens[t[p]] - lens[q[p]];
        if (delta < -kk || lens[q[p]] == 0 || lens[t[p]] == 0) continue;
        if (!hw_words(hw_locate_rows(delta, kk))) {
            g_last_error = "isocon_hw_pairs: band of " + std::to_string(hw_locate_rows(delta, kk)) + " diagonals not supported (limit 512)";
            return ISOCON_E_UNSUPPORTED;
        }
        run.push_back((uint32_t)p);
    }
    g_hw_stats[HS_NEED_KERNEL] = (double)run.size();
    if (run.empty()) return ISOCON_OK;
    HostClock clk;
    clk.lap("hw: classify");
    ScratchPool *pl = &g_scratch;
    DevBuf d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT), d_trace(pl, SLOT_HW_TRACE);
    DevBuf d_tq(pl, SLOT_HW_TILEQ), d_lp(pl, SLOT_HW_LANES);
    int rc;
    if ((rc = d_t.alloc(n_pairs * 4)) || (rc = d_k.alloc(n_pairs * 4)) || (rc = d_he.alloc(n_pairs * 8))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_t.p, t, n_pairs * 4));
    ISO_HIP_CHECK(copy_h2d(d_k.p, k, n_pairs * 4));
    EventTimer tm;
    auto upload_tiles = [&](const std::vector<uint32_t> &tq, const std::vector<uint32_t> &lp, HwTileIn &in) -> int {
        int r;
        if ((r = d_tq.alloc(tq.size() * 4)) || (r = d_lp.alloc(lp.size() * 4))) return r;
        ISO_HIP_CHECK(copy_h2d(d_tq.p, tq.data(), tq.size() * 4));
        ISO_HIP_CHECK(copy_h2d(d_lp.p, lp.data(), lp.size() * 4));
        in.tile_q = d_tq.as<uint32_t>(); in.lane_pair = d_lp.as<uint32_t>();
        in.pt = d_t.as<uint32_t>(); in.pk = d_k.as<int32_t>(); in.n_tiles = (uint32_t)tq.size();
        return ISOCON_OK;
    };
    // ---- LOCATE: distance and first end of every pair ----
    {
        HwTiles tiles;
        hw_build_tiles(run, q, n,
                       [&](uint32_t p) { return hw_words(hw_locate_rows(lens[t[p]] - lens[q[p]], k[p])); },
                       [&](uint32_t p, int32_t &dmax, int32_t &kmax, int Wc) {
                           const int32_t d2 = std::max(dmax, lens[t[p]] - lens[q[p]]), k2 = std::max(kmax, k[p]);
                           if (hw_locate_rows(d2, k2) > 64 * Wc) return false;
                           dmax = d2; kmax = k2;
                           return true;
                       }, tiles);
        clk.lap("hw: locate tiles (host)");
        for (int c = 0; c < 4; ++c) {
            g_hw_stats[HS_LOCATE + c] = (double)tiles.tile_q[c].size();
            if (tiles.tile_q[c].empty()) continue;
            HwTileIn in{};
            if ((rc = upload_tiles(tiles.tile_q[c], tiles.lane_pair[c], in))) return rc;
            tm.start();
            rc = c == 0 ? hw_launch_locate<1>(s, in, d_he.as<int32_t>()) : c == 1 ? hw_launch_locate<2>(s, in, d_he.as<int32_t>())
               : c == 2 ? hw_launch_locate<4>(s, in, d_he.as<int32_t>()) : hw_launch_locate<8>(s, in, d_he.as<int32_t>());
            if (rc) return rc;
            tm.stop();
        }
    }
    clk.lap("hw: locate kernels");
    std::vector<int32_t> he(n_pairs * 2);
    ISO_HIP_CHECK(copy_d2h(he.data(), d_he.p, n_pairs * 8));
    std::vector<uint32_t> hits;
    for (uint32_t p : run) {
        const int32_t h = he[(size_t)p * 2];
        if (h < -1) { g_last_error = "isocon_hw_pairs: internal status " + std::to_string(h) + " (locate) for pair " + std::to_string(p); return ISOCON_E_HIP; }
        if (h >= 0) hits.push_back(p);
    }
    if (clk.on) fprintf(stderr, "[isocon] hw: %zu pairs, %zu need a kernel, %zu hits\n", (size_t)n_pairs, run.size(), hits.size());
    clk.lap("hw: he download + hit list");
    g_hw_stats[HS_HITS] = (double)hits.size();
    if (hits.empty()) { if (kernel_ms) *kernel_ms = tm.total; return ISOCON_OK; }
    // ---- START + TRACE + walk for the hits: smallest start, terminal insertion runs ----
    if ((rc = d_out.alloc(n_pairs * 20))) return rc;
    {
        HwTiles tiles;
        hw_build_tiles(hits, q, n,
                       [&](uint32_t p) { return hw_words(2 * k[p] + 1); },
                       [&](uint32_t p, int32_t &dmax, int32_t &kmax, int Wc) {
                           const int32_t k2 = std::max(kmax, k[p]);
                           if (2 * k2 + 1 > 64 * Wc) return false;
                           dmax = 0; kmax = k2;
                           return true;
                       }, tiles);
        clk.lap("hw: finish tiles (host)");
        const uint32_t trace_cols = (uint32_t)s->maxlen + 1;
        for (int c = 0; c < 4; ++c) {
            g_hw_stats[HS_FINISH + c] = (double)tiles.tile_q[c].size();
            if (tiles.tile_q[c].empty()) continue;
            const int Wc = 1 << c;
            HwTileIn in{};
            if ((rc = upload_tiles(tiles.tile_q[c], tiles.lane_pair[c], in))) return rc;
            // one wavefront per tile in flight, each with its own column store: as many as 16 per CU, bounded by memory
            const uint64_t per_block = hw_finish_store_bytes(Wc, trace_cols);
            size_t free_b = 0, total_b = 0;
            uint64_t budget = (uint64_t)12 << 30;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min<uint64_t>(budget, (uint64_t)free_b / 3);
            const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(in.n_tiles, hw_finish_grid_cap(Wc)), budget / per_block));
            g_hw_stats[HS_GRID + c] = (double)grid;
            if ((rc = d_trace.alloc((size_t)grid * per_block))) return rc;
            tm.start();
            rc = c == 0 ? hw_launch_finish<1>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
               : c == 1 ? hw_launch_finish<2>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
               : c == 2 ? hw_launch_finish<4>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
                        : hw_launch_finish<8>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>());
            if (rc) return rc;
            tm.stop();                                  // also the fence before the column store is reused / regrown
        }
    }
    clk.lap("hw: finish kernels");
    // only the hits' rows were written on the device: fetch the whole array once and pick them (one large copy beats many small)
    std::vector<int32_t> res(n_pairs * 5);
    ISO_HIP_CHECK(copy_d2h(res.data(), d_out.p, n_pairs * 20));
    for (uint32_t p : hits) {
        const int32_t *r = res.data() + (size_t)p * 5;
        if (r[0] < -1) { g_last_error = "isocon_hw_pairs: internal status " + std::to_string(r[0]) + " for pair " + std::to_string(p); return ISOCON_E_HIP; }
        int32_t *o = out + (size_t)p * 5;
        for (int i = 0; i < 5; ++i) o[i] = r[i];
    }
    clk.lap("hw: results");
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

template <int STAGE>
int hw_device_tiles(isocon_store *st, uint64_t n_pairs, const uint32_t *d_q, const uint32_t *d_t, const int32_t *d_k, int32_t *d_he, int32_t *d_out,
                    uint32_t *d_key, uint32_t *d_hist, uint32_t *d_cursor, uint32_t *d_tbase, uint32_t n_keys, uint32_t *d_tq, uint32_t *d_lp, uint32_t max_tiles,
                    uint32_t *d_cls, HwTileCounters *d_ctr, HwTileCounters &ctr)
{
    ISO_HIP_CHECK(hipMemsetAsync(d_hist, 0, (size_t)n_keys * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_cursor, 0, (size_t)n_keys * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_ctr, 0, sizeof(HwTileCounters), 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_lp, 0xff, (size_t)max_tiles * 256, 0));
    const unsigned pb = (unsigned)((n_pairs + 255) / 256);
    hipLaunchKernelGGL((k_hwt_keys<STAGE>), dim3(pb), dim3(256), 0, 0, st->dev, d_q, d_t, d_k, (unsigned long long)n_pairs, d_he, d_out, d_key, d_hist, d_ctr);
    { int rc = device_exscan<6, uint32_t>(&g_scratch, d_hist, n_keys, d_tbase); if (rc) return rc; }
    hipLaunchKernelGGL(k_hwt_scatter, dim3(pb), dim3(256), 0, 0, d_key, (unsigned long long)n_pairs, d_tbase, d_cursor, d_tq, d_lp);
    hipLaunchKernelGGL((k_hwt_classes<STAGE>), dim3((max_tiles + 3) / 4), dim3(256), 0, 0, st->dev, d_tq, d_lp, d_t, d_k, max_tiles, d_tbase + n_keys, d_cls, d_ctr);
    ISO_HIP_CHECK(hipGetLastError());
    ISO_HIP_CHECK(hipMemcpy(&ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost));
    return ISOCON_OK;
}

// The rows of pair lists that are already in device memory (d_q, d_t, d_k: n_pairs entries each), tiles built on the device
// (hw_tiles.hpp): *d_rows = the (n_pairs, 5) result in the pool's SLOT_HW_OUT, good until the next call that takes that slot.
// Returns ISOCON_E_UNSUPPORTED with *retry_host set when only the host's greedy cut can form the tiles.
int hw_pairs_device_core(isocon_store *s, const uint32_t *d_q, const uint32_t *d_t, const int32_t *d_k, uint64_t n_pairs, int32_t **d_rows, float *kernel_ms,
                         bool *retry_host)
{
    *retry_host = false;
    const uint32_t n = s->dev.n;
    hw_stats_route(1, n_pairs);
    g_hw_stats[HS_NEED_KERNEL] = g_hw_stats[HS_HITS] = -1;          // (counted by hw_pairs_device_tiles, which has the lists on the host)
    if ((uint64_t)n * 4 >= 0xfffffff0ull) { *retry_host = true; return ISOCON_E_UNSUPPORTED; }
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT), d_trace(pl, SLOT_HW_TRACE);
    DevBuf d_tq(pl, SLOT_HW_TILEQ), d_lp(pl, SLOT_HW_LANES), d_key(pl, SLOT_HW_KEY), d_hist(pl, SLOT_HW_HIST), d_cursor(pl, SLOT_HW_CURSOR),
        d_tbase(pl, SLOT_HW_TBASE), d_cls(pl, SLOT_HW_CLS), d_ctr(pl, SLOT_HW_CTR);
    const uint32_t n_keys = n * 4u;
    const uint64_t max_tiles64 = n_pairs / 64 + std::min<uint64_t>(n_pairs, n_keys) + 1;
    if (max_tiles64 > 0x7fffff00ull) { *retry_host = true; return ISOCON_E_UNSUPPORTED; }
    const uint32_t max_tiles = (uint32_t)max_tiles64;
    int rc;
    if ((rc = d_he.alloc(n_pairs * 8)) ||
        (rc = d_out.alloc(n_pairs * 20)) || (rc = d_key.alloc(n_pairs * 4)) || (rc = d_hist.alloc((size_t)n_keys * 4)) || (rc = d_cursor.alloc((size_t)n_keys * 4)) ||
        (rc = d_tbase.alloc(((size_t)n_keys + 1) * 4)) || (rc = d_tq.alloc((size_t)max_tiles * 4)) || (rc = d_lp.alloc((size_t)max_tiles * 256)) ||
        (rc = d_cls.alloc((size_t)max_tiles * 16)) || (rc = d_ctr.alloc(sizeof(HwTileCounters))))
        return rc;
    EventTimer tm;
    HwTileCounters ctr;
    auto flag_error = [&](uint32_t flags) -> int {
        if (flags & HWT_ERR_INDEX) return ISOCON_E_ARG;
        if (flags & HWT_ERR_K_NEGATIVE) { g_last_error = "isocon_hw_pairs: k must be >= 0 (the band is derived from it)"; return ISOCON_E_ARG; }
        if (flags & HWT_ERR_K_LARGE) return ISOCON_E_UNSUPPORTED;
        if (flags & HWT_ERR_BAND) { g_last_error = "isocon_hw_pairs: a pair's band needs more than 512 diagonals (not supported)"; return ISOCON_E_UNSUPPORTED; }
        if (flags & HWT_ERR_TILE_BAND) { *retry_host = true; return ISOCON_E_UNSUPPORTED; }
        if (flags & HWT_ERR_STATUS) { g_last_error = "isocon_hw_pairs: internal status from a kernel"; return ISOCON_E_HIP; }
        return ISOCON_OK;
    };
    auto tile_in = [&](int c, const HwTileCounters &cc) {
        HwTileIn in{};
        in.tile_q = d_tq.as<uint32_t>(); in.lane_pair = d_lp.as<uint32_t>(); in.pt = d_t; in.pk = d_k;
        in.n_tiles = cc.cls[c]; in.tile_list = d_cls.as<uint32_t>() + (size_t)c * max_tiles; in.flags = &d_ctr.as<HwTileCounters>()->flags;
        return in;
    };
    // ---- LOCATE ----
    tm.start();
    if ((rc = hw_device_tiles<0>(s, n_pairs, d_q, d_t, d_k, d_he.as<int32_t>(), d_out.as<int32_t>(), d_key.as<uint32_t>(),
                                 d_hist.as<uint32_t>(), d_cursor.as<uint32_t>(), d_tbase.as<uint32_t>(), n_keys, d_tq.as<uint32_t>(), d_lp.as<uint32_t>(), max_tiles,
                                 d_cls.as<uint32_t>(), d_ctr.as<HwTileCounters>(), ctr)))
        return rc;
    tm.stop();
    if ((rc = flag_error(ctr.flags))) return rc;
    clk.lap("hw: locate tiles (device)");
    tm.start();
    for (int c = 0; c < 4; ++c) {
        g_hw_stats[HS_LOCATE + c] = (double)ctr.cls[c];
        if (!ctr.cls[c]) continue;
        const HwTileIn in = tile_in(c, ctr);
        rc = c == 0 ? hw_launch_locate<1>(s, in, d_he.as<int32_t>()) : c == 1 ? hw_launch_locate<2>(s, in, d_he.as<int32_t>())
           : c == 2 ? hw_launch_locate<4>(s, in, d_he.as<int32_t>()) : hw_launch_locate<8>(s, in, d_he.as<int32_t>());
        if (rc) return rc;
    }
    // ---- START + TRACE + walk for the hits ----
    if ((rc = hw_device_tiles<1>(s, n_pairs, d_q, d_t, d_k, d_he.as<int32_t>(), d_out.as<int32_t>(), d_key.as<uint32_t>(),
                                 d_hist.as<uint32_t>(), d_cursor.as<uint32_t>(), d_tbase.as<uint32_t>(), n_keys, d_tq.as<uint32_t>(), d_lp.as<uint32_t>(), max_tiles,
                                 d_cls.as<uint32_t>(), d_ctr.as<HwTileCounters>(), ctr)))
        return rc;
    tm.stop();
    if ((rc = flag_error(ctr.flags))) return rc;
    clk.lap("hw: locate kernels + finish tiles (device)");
    const uint32_t trace_cols = (uint32_t)s->maxlen + 1;
    for (int c = 0; c < 4; ++c) {
        g_hw_stats[HS_FINISH + c] = (double)ctr.cls[c];
        if (!ctr.cls[c]) continue;
        const int Wc = 1 << c;
        const HwTileIn in = tile_in(c, ctr);
        const uint64_t per_block = hw_finish_store_bytes(Wc, trace_cols);
        size_t free_b = 0, total_b = 0;
        uint64_t budget = (uint64_t)12 << 30;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min<uint64_t>(budget, (uint64_t)free_b / 3);
        const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(in.n_tiles, hw_finish_grid_cap(Wc)), budget / per_block));
        g_hw_stats[HS_GRID + c] = (double)grid;
        if ((rc = d_trace.alloc((size_t)grid * per_block))) return rc;
        tm.start();
        rc = c == 0 ? hw_launch_finish<1>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
           : c == 1 ? hw_launch_finish<2>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
           : c == 2 ? hw_launch_finish<4>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>())
                    : hw_launch_finish<8>(s, in, grid, d_he.as<int32_t>(), d_trace.as<uint64_t>(), trace_cols, d_out.as<int32_t>());
        if (rc) return rc;
        tm.stop();                                  // also the fence before the column store is reused / regrown
    }
    clk.lap("hw: finish kernels");
    ISO_HIP_CHECK(hipMemcpy(&ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
    if ((rc = flag_error(ctr.flags))) return rc;
    *d_rows = d_out.as<int32_t>();
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

// Tiles built on the device: the caller's pair arrays go up once, the (n_pairs, 5) result comes down once.
int hw_pairs_device_tiles(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out, float *kernel_ms,
                          bool *retry_host)
{
    *retry_host = false;
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K);
    int rc;
    if ((rc = d_q.alloc(n_pairs * 4)) || (rc = d_t.alloc(n_pairs * 4)) || (rc = d_k.alloc(n_pairs * 4))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_q.p, q, n_pairs * 4));
    ISO_HIP_CHECK(copy_h2d(d_t.p, t, n_pairs * 4));
    ISO_HIP_CHECK(copy_h2d(d_k.p, k, n_pairs * 4));
    clk.lap("hw: pair arrays up");
    int32_t *d_rows = nullptr;
    if ((rc = hw_pairs_device_core(s, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_k.as<int32_t>(), n_pairs, &d_rows, kernel_ms, retry_host))) return rc;
    ISO_HIP_CHECK(copy_d2h(out, d_rows, n_pairs * 20));
    clk.lap("hw: results down");
    // (isocon_hw_last_stats: the pairs the device classed as needing a kernel -- the rule of k_hwt_keys<0> -- and the hits among the rows)
    const std::vector<int32_t> &lens = s->lens;
    uint64_t need = 0, nhits = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const int32_t lq = lens[q[p]], lt = lens[t[p]];
        need += !(lt - lq < -k[p] || lq == 0 || lt == 0);
        nhits += out[p * 5] >= 0;
    }
    g_hw_stats[HS_NEED_KERNEL] = (double)need;
    g_hw_stats[HS_HITS] = (double)nhits;
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_hw_last_stats(double *out, int32_t cap)
{
    if (!out || cap < 0) return 0;
    const int k = cap < (int)HS_COUNT ? cap : (int)HS_COUNT;
    for (int i = 0; i < k; ++i) out[i] = g_hw_stats[i];
    return k;
}

extern "C" int isocon_hw_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                               int32_t *out, float *kernel_ms)
{
    for (double &x : g_hw_stats) x = 0;
    if (!s || (n_pairs && (!q || !t || !k || !out))) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    if (n_pairs > 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    if (n_pairs >= 2048 && !variant("hw_host_tiles")) {
        bool retry_host = false;
        const int rc = hw_pairs_device_tiles(s, q, t, k, n_pairs, out, kernel_ms, &retry_host);
        if (!retry_host) return rc;
        g_hw_stats[HS_RETRIED_HOST] = 1;
        if (kernel_ms) *kernel_ms = 0.f;
    }
    return hw_pairs_host_tiles(s, q, t, k, n_pairs, out, kernel_ms);
}
