// hw_loc_host.inc -- host side of isocon_hw_locations (included by isocon_hip.hip after hw_host.inc, whose HwDriver it runs on): LOCATE as
// on the device route of isocon_hw_pairs (build_device<0>, k_hw_locate), then ENDS twice (count, fill) and START once on the kernels of
// hw_loc.hpp.  The stages hand each other device arrays; the host reads the tile counters of every stage (as hw_pairs_device_core does) and
// the total that sizes the output.  Only where a run of 64 pairs of one query has a common window above 512 diagonals although every pair
// fits on its own are the tiles of that stage cut on the host (cut_host, the cut of hw_pairs_host_tiles).

namespace {

// isocon_hw_locations_last_stats: pairs, hits, locations, then the tiles per class (1, 2, 4, 8 window words) of the three stages
enum { HL_PAIRS = 0, HL_HITS, HL_LOCATIONS, HL_HOST_CUTS, HL_LOCATE, HL_ENDS = HL_LOCATE + 4, HL_STARTS = HL_ENDS + 4, HL_COUNT = HL_STARTS + 4 };
thread_local double g_hw_loc_stats[HL_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int hw_launch_ends(isocon_store *st, int c, const HwTileIn &in, bool fill, uint32_t *d_cnt, const unsigned long long *d_ptr, const HwLocList &E)
{
    return hw_for_words(c, [&](auto w) -> int {
        constexpr int W = decltype(w)::value;
        if (fill) hipLaunchKernelGGL((k_hw_ends<W, 1>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, E);
        else hipLaunchKernelGGL((k_hw_ends<W, 0>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, E);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

int hw_launch_starts(isocon_store *st, int c, const HwTileIn &in, const int32_t *d_he, int32_t *d_locs)
{
    return hw_for_words(c, [&](auto w) -> int {
        hipLaunchKernelGGL((k_hw_starts<decltype(w)::value>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_he, d_locs);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

}  // namespace

extern "C" int isocon_hw_locations_last_stats(double *out, int32_t cap) { return copy_last_stats(g_hw_loc_stats, HL_COUNT, out, cap); }

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
    HwDriver drv(s, pl);
    DevBuf d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT);
    DevBuf d_thr(pl, SLOT_HWL_THR), d_cnt(pl, SLOT_HWL_CNT), d_ptr(pl, SLOT_HWL_PTR), d_eq(pl, SLOT_HWL_EQ), d_et(pl, SLOT_HWL_ET), d_eh(pl, SLOT_HWL_EH),
        d_ehe(pl, SLOT_HWL_EHE), d_locs(pl, SLOT_HWL_LOCS);
    int rc;
    if ((rc = d_q.upload(q, n_pairs * 4)) || (rc = d_t.upload(t, n_pairs * 4)) || (rc = d_k.upload(k, n_pairs * 4)) || (rc = d_he.alloc(n_pairs * 8)) ||
        (rc = d_out.alloc(n_pairs * 20)) || (rc = d_thr.alloc(n_pairs * 4)) || (rc = d_cnt.alloc(n_pairs * 4)) || (rc = d_ptr.alloc((n_pairs + 1) * 8)) ||
        (rc = drv.size(n_pairs)))
        return rc;
    clk.lap("hw locations: pair arrays up");
    EventTimer tm;
    const char *const entry = "isocon_hw_locations";
    // The tiles of a LOCATE-shaped stage over (d_q, d_t, d_kk); STAGE names the builder's rule.  thr: the host's copy of d_kk, or nullptr: it
    // is fetched, and only when the tiles must be cut on the host.
    auto locate_shaped = [&](auto stage, const int32_t *d_kk, int32_t *d_khe, const int32_t *thr, HwStageTiles &tl) -> int {
        int r;
        if ((r = drv.build_device<decltype(stage)::value>(n_pairs, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_kk, d_khe, d_out.as<int32_t>(), tl))) return r;
        if ((r = hw_flag_error(tl.ctr.flags, entry, nullptr)) || !(tl.ctr.flags & HWT_ERR_TILE_BAND)) return r;
        std::vector<int32_t> fetched;
        if (!thr) {
            fetched.resize(n_pairs);
            if (copy_d2h(fetched.data(), d_kk, n_pairs * 4) != hipSuccess) { g_last_error = "isocon_hw_locations: internal status (tile band)"; return ISOCON_E_HIP; }
            thr = fetched.data();
        }
        g_hw_loc_stats[HL_HOST_CUTS] += 1;
        std::vector<uint32_t> idx;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const int32_t lq = lens[q[p]], lt = lens[t[p]];
            if (thr[p] >= 0 && lq > 0 && lt > 0 && lt - lq >= -thr[p]) idx.push_back((uint32_t)p);
        }
        drv.cut_host(idx, q, HwLocateCut{lens.data(), q, t, thr}, tl);
        ISO_HIP_CHECK(hipMemsetAsync(drv.flags(), 0, 4, 0));
        return ISOCON_OK;
    };
    auto kernel_flags = [&]() -> int {
        uint32_t flags = 0;
        ISO_HIP_CHECK(memcpy_wait(&flags, drv.flags(), 4, hipMemcpyDeviceToHost));
        return hw_flag_error(flags, entry, nullptr);
    };
    // ---- LOCATE: distance and first end of every pair (the first stage of hw_pairs_device_core) ----
    HwStageTiles tl;
    tm.start();
    if ((rc = locate_shaped(std::integral_constant<int, 0>(), d_k.as<int32_t>(), d_he.as<int32_t>(), k, tl))) return rc;
    if ((rc = drv.for_classes(tl, d_t.as<uint32_t>(), d_k.as<int32_t>(), g_hw_loc_stats + HL_LOCATE,
                              [&](int c, const HwTileIn &in) { return hw_launch_locate(s, c, in, d_he.as<int32_t>()); })))
        return rc;
    hipLaunchKernelGGL(k_hw_loc_prep, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, 0, d_he.as<int32_t>(), (unsigned long long)n_pairs, d_thr.as<int32_t>(),
                       d_cnt.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    // ---- ENDS, first run: how many columns of every hit attain its distance ----
    HwLocList E{};
    if ((rc = locate_shaped(std::integral_constant<int, 2>(), d_thr.as<int32_t>(), nullptr, nullptr, tl))) return rc;
    auto ends = [&](bool fill) -> int {
        return drv.for_classes(tl, d_t.as<uint32_t>(), d_thr.as<int32_t>(), fill ? nullptr : g_hw_loc_stats + HL_ENDS, [&](int c, const HwTileIn &in) {
            return hw_launch_ends(s, c, in, fill, d_cnt.as<uint32_t>(), d_ptr.as<unsigned long long>(), E);
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
    if ((rc = drv.size(total))) return rc;
    HwStageTiles ts;
    if ((rc = drv.build_device<1>(total, E.q, E.t, E.h, E.he, d_out.as<int32_t>(), ts)) || (rc = hw_flag_error(ts.ctr.flags, entry, nullptr))) return rc;
    // (the builder keys by 2 h + 1, which a tile's largest h cannot push out of its class)
    if (ts.ctr.flags & HWT_ERR_TILE_BAND) { g_last_error = "isocon_hw_locations: internal status (tile band)"; return ISOCON_E_HIP; }
    if ((rc = drv.for_classes(ts, E.t, E.h, g_hw_loc_stats + HL_STARTS,
                              [&](int c, const HwTileIn &in) { return hw_launch_starts(s, c, in, E.he, d_locs.as<int32_t>()); })))
        return rc;
    tm.stop();
    clk.lap("hw locations: ends (fill), starts");
    if ((rc = kernel_flags())) return rc;
    ISO_HIP_CHECK(copy_d2h(out_locs, d_locs.p, total * 8));
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}
