// hw_host.inc -- host side of isocon_hw_pairs (included by isocon_hip.hip), and the driver every entry on the banded infix kernels of
// hw.hpp and hw_loc.hpp runs on (HwDriver: the tiles of a stage, one launch per class, the finish stage).  Tiles are one query x up to 64
// targets; what the host decides about them without a device (the greedy cut, the finish grid) is in hw_plan.hpp.

namespace {

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

// f(std::integral_constant<int, W>()) for the window words W = 1, 2, 4, 8 of class c = 0 .. 3
template <class F>
int hw_for_words(int c, F f)
{
    switch (c) {
    case 0: return f(std::integral_constant<int, 1>());
    case 1: return f(std::integral_constant<int, 2>());
    case 2: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

int hw_launch_locate(isocon_store *st, int c, const HwTileIn &in, int32_t *d_he)
{
    return hw_for_words(c, [&](auto w) -> int {
        hipLaunchKernelGGL((k_hw_locate<decltype(w)::value>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_he);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

int hw_launch_finish(isocon_store *st, int c, const HwTileIn &in, uint32_t grid, const int32_t *d_he, uint64_t *d_trace, uint32_t trace_cols, int32_t *d_out)
{
    return hw_for_words(c, [&](auto w) -> int {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((k_hw_finish<W>), dim3(grid), dim3(64), hw_finish_lds(W), 0, st->dev, in, d_he, d_trace, trace_cols, d_out);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

// What the error flags of the tile builder and the kernels (HwTileCounters::flags) mean to `entry`.  retry_host: where to say that only the
// host's greedy cut can form the tiles; nullptr: the caller deals with HWT_ERR_TILE_BAND itself.
int hw_flag_error(uint32_t flags, const char *entry, bool *retry_host)
{
    if (flags & HWT_ERR_INDEX) return ISOCON_E_ARG;
    if (flags & HWT_ERR_K_NEGATIVE) { g_last_error = std::string(entry) + ": k must be >= 0 (the band is derived from it)"; return ISOCON_E_ARG; }
    if (flags & HWT_ERR_K_LARGE) return ISOCON_E_UNSUPPORTED;
    if (flags & HWT_ERR_BAND) { g_last_error = std::string(entry) + ": a pair's band needs more than 512 diagonals (not supported)"; return ISOCON_E_UNSUPPORTED; }
    if (retry_host && (flags & HWT_ERR_TILE_BAND)) { *retry_host = true; return ISOCON_E_UNSUPPORTED; }
    if (flags & HWT_ERR_STATUS) { g_last_error = std::string(entry) + ": internal status from a kernel"; return ISOCON_E_HIP; }
    return ISOCON_OK;
}

// the tiles of one stage: lists per class in device memory (HwDriver::build_device) or cut on the host (HwDriver::cut_host)
struct HwStageTiles {
    bool host = false;
    HwTileCounters ctr{};
    HwTiles cut;
    uint32_t count(int c) const { return host ? (uint32_t)cut.tile_q[c].size() : ctr.cls[c]; }
};

// The stages of one call.  A call that builds tiles on the device sizes the builder's arrays first (size()); its kernels then report
// through the counters' flag word and nothing fences its launches.  Without size() -- the host route of isocon_hw_pairs, which reads every
// row's status and waits behind every launch -- the kernels get no flag word.
struct HwDriver {
    isocon_store *s;
    DevBuf d_tq, d_lp, d_key, d_hist, d_cursor, d_tbase, d_cls, d_ctr, d_trace;
    uint32_t n_keys = 0, max_tiles = 0;
    HwDriver(isocon_store *st, ScratchPool *pl)
        : s(st), d_tq(pl, SLOT_HW_TILEQ), d_lp(pl, SLOT_HW_LANES), d_key(pl, SLOT_HW_KEY), d_hist(pl, SLOT_HW_HIST), d_cursor(pl, SLOT_HW_CURSOR),
          d_tbase(pl, SLOT_HW_TBASE), d_cls(pl, SLOT_HW_CLS), d_ctr(pl, SLOT_HW_CTR), d_trace(pl, SLOT_HW_TRACE) {}
    uint32_t *flags() { return d_ctr.p ? &d_ctr.as<HwTileCounters>()->flags : nullptr; }

    // the builder's arrays for a list of `count` entries; ISOCON_E_UNSUPPORTED: more keys or tiles than it can index
    int size(uint64_t count)
    {
        if ((uint64_t)s->dev.n * 4 >= 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
        n_keys = s->dev.n * 4u;
        const uint64_t mt = count / 64 + std::min<uint64_t>(count, n_keys) + 1;
        if (mt > 0x7fffff00ull) return ISOCON_E_UNSUPPORTED;
        max_tiles = (uint32_t)mt;
        int rc;
        if ((rc = d_key.alloc(count * 4)) || (rc = d_hist.alloc((size_t)n_keys * 4)) || (rc = d_cursor.alloc((size_t)n_keys * 4)) ||
            (rc = d_tbase.alloc(((size_t)n_keys + 1) * 4)) || (rc = d_tq.alloc((size_t)max_tiles * 4)) || (rc = d_lp.alloc((size_t)max_tiles * 256)) ||
            (rc = d_cls.alloc((size_t)max_tiles * 16)) || (rc = d_ctr.alloc(sizeof(HwTileCounters))))
            return rc;
        return ISOCON_OK;
    }

    // tiles of the list (d_q, d_t, d_k) on the device (hw_tiles.hpp; STAGE names the builder's rule), tl.ctr = the stage's counters
    template <int STAGE>
    int build_device(uint64_t count, const uint32_t *d_q, const uint32_t *d_t, const int32_t *d_k, int32_t *d_he, int32_t *d_out, HwStageTiles &tl)
    {
        HwTileCounters *ctr = d_ctr.as<HwTileCounters>();
        uint32_t *hist = d_hist.as<uint32_t>(), *cursor = d_cursor.as<uint32_t>(), *tbase = d_tbase.as<uint32_t>(), *tq = d_tq.as<uint32_t>(), *lp = d_lp.as<uint32_t>();
        tl.host = false;
        ISO_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n_keys * 4, 0));
        ISO_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)n_keys * 4, 0));
        ISO_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof(HwTileCounters), 0));
        ISO_HIP_CHECK(hipMemsetAsync(lp, 0xff, (size_t)max_tiles * 256, 0));
        const unsigned pb = (unsigned)((count + 255) / 256);
        hipLaunchKernelGGL((k_hwt_keys<STAGE>), dim3(pb), dim3(256), 0, 0, s->dev, d_q, d_t, d_k, (unsigned long long)count, d_he, d_out, d_key.as<uint32_t>(), hist, ctr);
        if (int rc = device_exscan<6, uint32_t>(&g_scratch, hist, n_keys, tbase)) return rc;
        hipLaunchKernelGGL(k_hwt_scatter, dim3(pb), dim3(256), 0, 0, d_key.as<uint32_t>(), (unsigned long long)count, tbase, cursor, tq, lp);
        hipLaunchKernelGGL((k_hwt_classes<STAGE>), dim3((max_tiles + 3) / 4), dim3(256), 0, 0, s->dev, tq, lp, d_t, d_k, max_tiles, tbase + n_keys, d_cls.as<uint32_t>(), ctr);
        ISO_HIP_CHECK(hipGetLastError());
        return read_counters(tl.ctr);
    }
    int read_counters(HwTileCounters &ctr)
    {
        ISO_HIP_CHECK(hipMemcpy(&ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost));
        return ISOCON_OK;
    }

    // tiles of the pairs `idx` of the caller's arrays, cut on the host (two counting sorts and a greedy cut, hw_build_tiles): small calls,
    // and calls where a run of 64 pairs of one query has a common window wider than 512 diagonals although every pair fits on its own
    template <class Rule>
    void cut_host(const std::vector<uint32_t> &idx, const uint32_t *q, const Rule &rule, HwStageTiles &tl)
    {
        tl.host = true;
        tl.cut = HwTiles();
        hw_build_tiles(idx, q, s->dev.n, rule, tl.cut);
    }

    // launch(c, in) for every class c that has tiles; stat[c] = its tiles (stat may be nullptr)
    template <class Launch>
    int for_classes(const HwStageTiles &tl, const uint32_t *d_t, const int32_t *d_k, double *stat, Launch launch)
    {
        for (int c = 0; c < 4; ++c) {
            if (stat) stat[c] = (double)tl.count(c);
            if (!tl.count(c)) continue;
            HwTileIn in{};
            in.pt = d_t; in.pk = d_k; in.n_tiles = tl.count(c); in.flags = flags();
            int rc;
            if (tl.host) {
                const std::vector<uint32_t> &tq = tl.cut.tile_q[c], &lp = tl.cut.lane_pair[c];
                if (flags()) ISO_HIP_CHECK(device_wait());          // the launch before may still read the tiles these replace
                if ((rc = d_tq.upload(tq.data(), tq.size() * 4)) || (rc = d_lp.upload(lp.data(), lp.size() * 4))) return rc;
            } else in.tile_list = d_cls.as<uint32_t>() + (size_t)c * max_tiles;
            in.tile_q = d_tq.as<uint32_t>(); in.lane_pair = d_lp.as<uint32_t>();
            if ((rc = launch(c, in))) return rc;
        }
        return ISOCON_OK;
    }

    // START + TRACE + walk for the hits of he (smallest start, terminal insertion runs), one launch per class of `tl`; stats = g_hw_stats
    int finish_stage(const HwStageTiles &tl, const uint32_t *d_t, const int32_t *d_k, const int32_t *d_he, int32_t *d_out, EventTimer &tm, double *stats)
    {
        const uint32_t trace_cols = (uint32_t)s->maxlen + 1;
        return for_classes(tl, d_t, d_k, stats + HS_FINISH, [&](int c, const HwTileIn &in) -> int {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = ~(size_t)0;          // (then the fixed bound alone)
            const uint32_t grid = hw_finish_grid(in.n_tiles, 1 << c, trace_cols, free_b);
            stats[HS_GRID + c] = (double)grid;
            int rc;
            if ((rc = d_trace.alloc((size_t)grid * hw_finish_store_bytes(1 << c, trace_cols)))) return rc;
            tm.start();
            if ((rc = hw_launch_finish(s, c, in, grid, d_he, d_trace.as<uint64_t>(), trace_cols, d_out))) return rc;
            tm.stop();                                  // also the fence before the column store is reused / regrown
            return ISOCON_OK;
        });
    }
};

// Tiles cut on the host: small calls, and the retry of a call whose tiles the device could not form.
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
        if (!hwt_words(hw_locate_rows(delta, kk))) {
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
    HwDriver drv(s, pl);
    DevBuf d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT);
    int rc;
    if ((rc = d_t.upload(t, n_pairs * 4)) || (rc = d_k.upload(k, n_pairs * 4)) || (rc = d_he.alloc(n_pairs * 8))) return rc;
    EventTimer tm;
    HwStageTiles tiles;
    // ---- LOCATE: distance and first end of every pair ----
    drv.cut_host(run, q, HwLocateCut{lens.data(), q, t, k}, tiles);
    clk.lap("hw: locate tiles (host)");
    if ((rc = drv.for_classes(tiles, d_t.as<uint32_t>(), d_k.as<int32_t>(), g_hw_stats + HS_LOCATE, [&](int c, const HwTileIn &in) -> int {
             tm.start();
             if (int r = hw_launch_locate(s, c, in, d_he.as<int32_t>())) return r;
             tm.stop();
             return ISOCON_OK;
         })))
        return rc;
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
    // ---- START + TRACE + walk for the hits ----
    if ((rc = d_out.alloc(n_pairs * 20))) return rc;
    drv.cut_host(hits, q, HwFinishCut{k}, tiles);
    clk.lap("hw: finish tiles (host)");
    if ((rc = drv.finish_stage(tiles, d_t.as<uint32_t>(), d_k.as<int32_t>(), d_he.as<int32_t>(), d_out.as<int32_t>(), tm, g_hw_stats))) return rc;
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

// The rows of pair lists that are already in device memory (d_q, d_t, d_k: n_pairs entries each), tiles built on the device
// (hw_tiles.hpp): *d_rows = the (n_pairs, 5) result in the pool's SLOT_HW_OUT, good until the next call that takes that slot.
// Returns ISOCON_E_UNSUPPORTED with *retry_host set when only the host's greedy cut can form the tiles.
int hw_pairs_device_core(isocon_store *s, const uint32_t *d_q, const uint32_t *d_t, const int32_t *d_k, uint64_t n_pairs, int32_t **d_rows, float *kernel_ms,
                         bool *retry_host)
{
    *retry_host = false;
    hw_stats_route(1, n_pairs);
    g_hw_stats[HS_NEED_KERNEL] = g_hw_stats[HS_HITS] = -1;          // (counted by hw_pairs_device_tiles, which has the lists on the host)
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    HwDriver drv(s, pl);
    DevBuf d_he_buf(pl, SLOT_HW_Q), d_out_buf(pl, SLOT_HW_OUT);
    int rc;
    if ((rc = drv.size(n_pairs))) { *retry_host = rc == ISOCON_E_UNSUPPORTED; return rc; }
    if ((rc = d_he_buf.alloc(n_pairs * 8)) || (rc = d_out_buf.alloc(n_pairs * 20))) return rc;
    int32_t *d_he = d_he_buf.as<int32_t>(), *d_out = d_out_buf.as<int32_t>();
    EventTimer tm;
    HwStageTiles tiles;
    // ---- LOCATE ----
    tm.start();
    if ((rc = drv.build_device<0>(n_pairs, d_q, d_t, d_k, d_he, d_out, tiles))) return rc;
    tm.stop();
    if ((rc = hw_flag_error(tiles.ctr.flags, "isocon_hw_pairs", retry_host))) return rc;
    clk.lap("hw: locate tiles (device)");
    tm.start();
    if ((rc = drv.for_classes(tiles, d_t, d_k, g_hw_stats + HS_LOCATE, [&](int c, const HwTileIn &in) { return hw_launch_locate(s, c, in, d_he); }))) return rc;
    // ---- START + TRACE + walk for the hits ----
    if ((rc = drv.build_device<1>(n_pairs, d_q, d_t, d_k, d_he, d_out, tiles))) return rc;
    tm.stop();
    if ((rc = hw_flag_error(tiles.ctr.flags, "isocon_hw_pairs", retry_host))) return rc;
    clk.lap("hw: locate kernels + finish tiles (device)");
    if ((rc = drv.finish_stage(tiles, d_t, d_k, d_he, d_out, tm, g_hw_stats))) return rc;
    clk.lap("hw: finish kernels");
    if ((rc = drv.read_counters(tiles.ctr)) || (rc = hw_flag_error(tiles.ctr.flags, "isocon_hw_pairs", retry_host))) return rc;
    *d_rows = d_out;
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

extern "C" int isocon_hw_last_stats(double *out, int32_t cap) { return copy_last_stats(g_hw_stats, HS_COUNT, out, cap); }

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
