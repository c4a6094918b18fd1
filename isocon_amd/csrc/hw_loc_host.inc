// hw_loc_host.inc -- host side of isocon_hw_locations (included by isocon_hip.hip after hw_host.inc): LOCATE through the device route of
// isocon_hw_pairs (hw_device_tiles<0>, k_hw_locate), then ENDS twice (count, fill) and START once on the kernels of hw_loc.hpp.  The
// stages hand each other device arrays; the host reads the tile counters of every stage (as hw_pairs_device_core does) and the total
// that sizes the output.  Only where a run of 64 pairs of one query has a common window above 512 diagonals although every pair fits on
// its own are the tiles of that stage cut on the host (hw_build_tiles, the cut of hw_pairs_host_tiles).

namespace {

// isocon_hw_locations_last_stats: pairs, hits, locations, then the tiles per class (1, 2, 4, 8 window words) of the three stages
enum { HL_PAIRS = 0, HL_HITS, HL_LOCATIONS, HL_HOST_CUTS, HL_LOCATE, HL_ENDS = HL_LOCATE + 4, HL_STARTS = HL_ENDS + 4, HL_COUNT = HL_STARTS + 4 };
thread_local double g_hw_loc_stats[HL_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// the tiles of one stage: lists per class in device memory (hw_device_tiles) or cut on the host
struct HwLocTiles {
    bool host = false;
    HwTileCounters ctr{};
    HwTiles cut;
    uint32_t count(int c) const { return host ? (uint32_t)cut.tile_q[c].size() : ctr.cls[c]; }
};

template <int W>
int hw_launch_ends(isocon_store *st, const HwTileIn &in, bool fill, uint32_t *d_cnt, const unsigned long long *d_ptr, const HwLocList &E)
{
    if (fill) hipLaunchKernelGGL((k_hw_ends<W, 1>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, E);
    else hipLaunchKernelGGL((k_hw_ends<W, 0>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, E);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

template <int W>
int hw_launch_starts(isocon_store *st, const HwTileIn &in, const int32_t *d_he, int32_t *d_locs)
{
    hipLaunchKernelGGL((k_hw_starts<W>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_he, d_locs);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_hw_locations_last_stats(double *out, int32_t cap)
{
    if (!out || cap < 0) return 0;
    const int k = cap < (int)HL_COUNT ? cap : (int)HL_COUNT;
    for (int i = 0; i < k; ++i) out[i] = g_hw_loc_stats[i];
    return k;
}

extern "C" int isocon_hw_locations(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out_ed,
                                   uint64_t *out_loc_ptr, int32_t *out_locs, uint64_t cap, uint64_t *needed, float *kernel_ms)
{
    for (double &x : g_hw_loc_stats) x = 0;
    if (!s || !out_loc_ptr || (n_pairs && (!q || !t || !k || !out_ed)) || (cap && !out_locs)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (needed) *needed = 0;
    out_loc_ptr[0] = 0;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    if (n_pairs > 0xfffffff0ull || (uint64_t)n * 4 >= 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    g_hw_loc_stats[HL_PAIRS] = (double)n_pairs;
    const std::vector<int32_t> &lens = s->lens;
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT);
    DevBuf d_tq(pl, SLOT_HW_TILEQ), d_lp(pl, SLOT_HW_LANES), d_key(pl, SLOT_HW_KEY), d_hist(pl, SLOT_HW_HIST), d_cursor(pl, SLOT_HW_CURSOR),
        d_tbase(pl, SLOT_HW_TBASE), d_cls(pl, SLOT_HW_CLS), d_ctr(pl, SLOT_HW_CTR);
    DevBuf d_thr(pl, SLOT_HWL_THR), d_cnt(pl, SLOT_HWL_CNT), d_ptr(pl, SLOT_HWL_PTR), d_eq(pl, SLOT_HWL_EQ), d_et(pl, SLOT_HWL_ET), d_eh(pl, SLOT_HWL_EH),
        d_ehe(pl, SLOT_HWL_EHE), d_locs(pl, SLOT_HWL_LOCS);
    const uint32_t n_keys = n * 4u;
    uint32_t max_tiles = 0;
    int rc;
    // the builder's arrays for a list of `count` entries
    auto size_tiles = [&](uint64_t count) -> int {
        const uint64_t mt = count / 64 + std::min<uint64_t>(count, n_keys) + 1;
        if (mt > 0x7fffff00ull) return ISOCON_E_UNSUPPORTED;
        max_tiles = (uint32_t)mt;
        int r;
        if ((r = d_key.alloc(count * 4)) || (r = d_hist.alloc((size_t)n_keys * 4)) || (r = d_cursor.alloc((size_t)n_keys * 4)) ||
            (r = d_tbase.alloc(((size_t)n_keys + 1) * 4)) || (r = d_tq.alloc((size_t)max_tiles * 4)) || (r = d_lp.alloc((size_t)max_tiles * 256)) ||
            (r = d_cls.alloc((size_t)max_tiles * 16)) || (r = d_ctr.alloc(sizeof(HwTileCounters))))
            return r;
        return ISOCON_OK;
    };
    if ((rc = d_q.upload(q, n_pairs * 4)) || (rc = d_t.upload(t, n_pairs * 4)) || (rc = d_k.upload(k, n_pairs * 4)) || (rc = d_he.alloc(n_pairs * 8)) ||
        (rc = d_out.alloc(n_pairs * 20)) || (rc = d_thr.alloc(n_pairs * 4)) || (rc = d_cnt.alloc(n_pairs * 4)) || (rc = d_ptr.alloc((n_pairs + 1) * 8)) ||
        (rc = size_tiles(n_pairs)))
        return rc;
    clk.lap("hw locations: pair arrays up");
    EventTimer tm;
    auto flag_error = [&](uint32_t flags) -> int {
        if (flags & HWT_ERR_INDEX) return ISOCON_E_ARG;
        if (flags & HWT_ERR_K_NEGATIVE) { g_last_error = "isocon_hw_locations: k must be >= 0 (the band is derived from it)"; return ISOCON_E_ARG; }
        if (flags & HWT_ERR_K_LARGE) return ISOCON_E_UNSUPPORTED;
        if (flags & HWT_ERR_BAND) { g_last_error = "isocon_hw_locations: a pair's band needs more than 512 diagonals (not supported)"; return ISOCON_E_UNSUPPORTED; }
        if (flags & HWT_ERR_STATUS) { g_last_error = "isocon_hw_locations: internal status from a kernel"; return ISOCON_E_HIP; }
        return ISOCON_OK;
    };
    // The tiles of a stage over (d_kq, d_kt, d_kk); STAGE names the builder's rule.  host_thr(): the host's copy of d_kk, asked for only when
    // the tiles must be cut on the host.
    auto build = [&](auto stage, uint64_t count, const uint32_t *d_kq, const uint32_t *d_kt, const int32_t *d_kk, int32_t *d_khe, auto host_thr,
                     HwLocTiles &tl) -> int {
        constexpr int STAGE = decltype(stage)::value;
        tl.host = false;
        int r;
        if ((r = hw_device_tiles<STAGE>(s, count, d_kq, d_kt, d_kk, d_khe, d_out.as<int32_t>(), d_key.as<uint32_t>(), d_hist.as<uint32_t>(), d_cursor.as<uint32_t>(),
                                        d_tbase.as<uint32_t>(), n_keys, d_tq.as<uint32_t>(), d_lp.as<uint32_t>(), max_tiles, d_cls.as<uint32_t>(),
                                        d_ctr.as<HwTileCounters>(), tl.ctr)))
            return r;
        if ((r = flag_error(tl.ctr.flags))) return r;
        if (!(tl.ctr.flags & HWT_ERR_TILE_BAND)) return ISOCON_OK;
        // (STAGE 1 keys by 2 h + 1, which a tile's largest h cannot push out of its class: only the LOCATE-shaped bands come here)
        const int32_t *thr = nullptr;
        if (STAGE == 1 || (r = host_thr(&thr)) || !thr) { g_last_error = "isocon_hw_locations: internal status (tile band)"; return r ? r : ISOCON_E_HIP; }
        tl.host = true;
        g_hw_loc_stats[HL_HOST_CUTS] += 1;
        std::vector<uint32_t> idx;
        for (uint64_t p = 0; p < count; ++p) {
            const int32_t lq = lens[q[p]], lt = lens[t[p]];
            if (thr[p] >= 0 && lq > 0 && lt > 0 && lt - lq >= -thr[p]) idx.push_back((uint32_t)p);
        }
        tl.cut = HwTiles();
        hw_build_tiles(idx, q, n,
                       [&](uint32_t p) { return hw_words(hw_locate_rows(lens[t[p]] - lens[q[p]], thr[p])); },
                       [&](uint32_t p, int32_t &dmax, int32_t &kmax, int Wc) {
                           const int32_t d2 = std::max(dmax, lens[t[p]] - lens[q[p]]), k2 = std::max(kmax, thr[p]);
                           if (hw_locate_rows(d2, k2) > 64 * Wc) return false;
                           dmax = d2; kmax = k2;
                           return true;
                       }, tl.cut);
        ISO_HIP_CHECK(hipMemsetAsync(&d_ctr.as<HwTileCounters>()->flags, 0, 4, 0));
        return ISOCON_OK;
    };
    // one launch per class of a stage's tiles
    auto for_classes = [&](HwLocTiles &tl, const uint32_t *d_kt, const int32_t *d_kk, int stat0, auto launch) -> int {
        for (int c = 0; c < 4; ++c) {
            if (stat0 >= 0) g_hw_loc_stats[stat0 + c] = (double)tl.count(c);
            if (!tl.count(c)) continue;
            HwTileIn in{};
            in.pt = d_kt; in.pk = d_kk; in.n_tiles = tl.count(c); in.flags = &d_ctr.as<HwTileCounters>()->flags;
            int r;
            if (tl.host) {
                const std::vector<uint32_t> &tq = tl.cut.tile_q[c], &lp = tl.cut.lane_pair[c];
                ISO_HIP_CHECK(device_wait());          // the launch before may still read the tiles these replace
                if ((r = d_tq.upload(tq.data(), tq.size() * 4)) || (r = d_lp.upload(lp.data(), lp.size() * 4))) return r;
            } else in.tile_list = d_cls.as<uint32_t>() + (size_t)c * max_tiles;
            in.tile_q = d_tq.as<uint32_t>(); in.lane_pair = d_lp.as<uint32_t>();
            if ((r = launch(c, in))) return r;
        }
        return ISOCON_OK;
    };
    auto kernel_flags = [&]() -> int {
        uint32_t flags = 0;
        ISO_HIP_CHECK(memcpy_wait(&flags, &d_ctr.as<HwTileCounters>()->flags, 4, hipMemcpyDeviceToHost));
        return flag_error(flags);
    };
    // ---- LOCATE: distance and first end of every pair (the first stage of hw_pairs_device_core) ----
    HwLocTiles tl;
    tm.start();
    if ((rc = build(std::integral_constant<int, 0>(), n_pairs, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_k.as<int32_t>(), d_he.as<int32_t>(),
                    [&](const int32_t **thr) { *thr = k; return (int)ISOCON_OK; }, tl)))
        return rc;
    if ((rc = for_classes(tl, d_t.as<uint32_t>(), d_k.as<int32_t>(), HL_LOCATE, [&](int c, const HwTileIn &in) {
             return c == 0 ? hw_launch_locate<1>(s, in, d_he.as<int32_t>()) : c == 1 ? hw_launch_locate<2>(s, in, d_he.as<int32_t>())
                  : c == 2 ? hw_launch_locate<4>(s, in, d_he.as<int32_t>()) : hw_launch_locate<8>(s, in, d_he.as<int32_t>());
         })))
        return rc;
    hipLaunchKernelGGL(k_hw_loc_prep, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, 0, d_he.as<int32_t>(), (unsigned long long)n_pairs, d_thr.as<int32_t>(),
                       d_cnt.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    // ---- ENDS, first run: how many columns of every hit attain its distance ----
    HwLocList E{};
    std::vector<int32_t> thr_host;
    if ((rc = build(std::integral_constant<int, 2>(), n_pairs, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_thr.as<int32_t>(), nullptr,
                    [&](const int32_t **thr) -> int {
                        thr_host.resize(n_pairs);
                        ISO_HIP_CHECK(copy_d2h(thr_host.data(), d_thr.p, n_pairs * 4));
                        *thr = thr_host.data();
                        return (int)ISOCON_OK;
                    }, tl)))
        return rc;
    auto ends = [&](bool fill) -> int {
        return for_classes(tl, d_t.as<uint32_t>(), d_thr.as<int32_t>(), fill ? -1 : HL_ENDS, [&](int c, const HwTileIn &in) {
            uint32_t *cn = d_cnt.as<uint32_t>();
            const unsigned long long *pp = d_ptr.as<unsigned long long>();
            return c == 0 ? hw_launch_ends<1>(s, in, fill, cn, pp, E) : c == 1 ? hw_launch_ends<2>(s, in, fill, cn, pp, E)
                 : c == 2 ? hw_launch_ends<4>(s, in, fill, cn, pp, E) : hw_launch_ends<8>(s, in, fill, cn, pp, E);
        });
    };
    if ((rc = ends(false))) return rc;
    if ((rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), (uint32_t)n_pairs, d_ptr.as<unsigned long long>()))) return rc;
    tm.stop();
    clk.lap("hw locations: locate, ends (count), scan");
    if ((rc = kernel_flags())) return rc;
    // ---- the caller's distances and row pointers; the total sizes everything behind ----
    ISO_HIP_CHECK(copy_d2h(out_ed, d_thr.p, n_pairs * 4));
    ISO_HIP_CHECK(copy_d2h(out_loc_ptr, d_ptr.p, (n_pairs + 1) * 8));
    const uint64_t total = out_loc_ptr[n_pairs];
    uint64_t hits = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) hits += out_ed[p] >= 0;
    g_hw_loc_stats[HL_HITS] = (double)hits;
    g_hw_loc_stats[HL_LOCATIONS] = (double)total;
    if (needed) *needed = total;
    if (kernel_ms) *kernel_ms = tm.total;
    if (total > cap) return ISOCON_E_CAPACITY;
    if (!total) return ISOCON_OK;
    if (total > 0xfffffff0ull) { g_last_error = "isocon_hw_locations: more than 2^32 - 16 locations in one call"; return ISOCON_E_UNSUPPORTED; }
    // ---- ENDS, second run: the expanded list, one entry per (pair, end) ----
    if ((rc = d_eq.alloc(total * 4)) || (rc = d_et.alloc(total * 4)) || (rc = d_eh.alloc(total * 4)) || (rc = d_ehe.alloc(total * 8)) || (rc = d_locs.alloc(total * 8)))
        return rc;
    E.q = d_eq.as<uint32_t>(); E.t = d_et.as<uint32_t>(); E.h = d_eh.as<int32_t>(); E.he = d_ehe.as<int32_t>();
    tm.start();
    if ((rc = ends(true))) return rc;
    // ---- START of every entry: tiles by (query, class of 2 h + 1), the builder of the finish stage on the expanded list ----
    if ((rc = kernel_flags())) return rc;          // (a wait as well: the builder's arrays are sized anew and its counters zeroed)
    if ((rc = size_tiles(total))) return rc;
    HwLocTiles ts;
    if ((rc = build(std::integral_constant<int, 1>(), total, E.q, E.t, E.h, E.he, [](const int32_t **) { return (int)ISOCON_OK; }, ts))) return rc;
    if ((rc = for_classes(ts, E.t, E.h, HL_STARTS, [&](int c, const HwTileIn &in) {
             return c == 0 ? hw_launch_starts<1>(s, in, E.he, d_locs.as<int32_t>()) : c == 1 ? hw_launch_starts<2>(s, in, E.he, d_locs.as<int32_t>())
                  : c == 2 ? hw_launch_starts<4>(s, in, E.he, d_locs.as<int32_t>()) : hw_launch_starts<8>(s, in, E.he, d_locs.as<int32_t>());
         })))
        return rc;
    tm.stop();
    clk.lap("hw locations: ends (fill), starts");
    if ((rc = kernel_flags())) return rc;
    ISO_HIP_CHECK(copy_d2h(out_locs, d_locs.p, total * 8));
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}
