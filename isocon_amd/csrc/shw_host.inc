// shw_host.inc -- host side of isocon_shw_locations and isocon_shw_path_pairs (included by isocon_hip.hip after hw_host.inc, whose HwDriver
// both run on, and nw_path_host.inc): prefix ("SHW") alignments of a pair list on the kernels of shw.hpp.  The distance stage runs in
// rounds of doubling thresholds (31, 63, 127, 255, each capped by the pair's own), one class of tiles wider every round, as edlib does
// for an unbounded search: a pair is settled once it hits, or misses at its own threshold.  Every stage builds its tiles on the device
// (hw_tiles.hpp, STAGE 3: a tile never outgrows the class of its largest threshold, so nothing is ever cut on the host); the host reads
// the round's pair count and the stage's tile counters, and the total that sizes the output.

namespace {

// isocon_shw_last_stats: pairs, hits, ends, rounds run, pairs entering each round, LOCATE tiles per class (summed over the rounds), ENDS
// tiles per class (1, 2, 4, 8 window words)
enum { SW_PAIRS = 0, SW_HITS, SW_ENDS, SW_ROUNDS, SW_ENTER, SW_LOCATE = SW_ENTER + 4, SW_ENDS_TILES = SW_LOCATE + 4, SW_COUNT = SW_ENDS_TILES + 4 };
thread_local double g_shw_stats[SW_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int shw_launch_locate(isocon_store *st, int c, const HwTileIn &in, int32_t *d_he)
{
    return hw_for_words(c, [&](auto w) -> int {
        hipLaunchKernelGGL((k_shw_locate<decltype(w)::value>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_he);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

int shw_launch_ends(isocon_store *st, int c, const HwTileIn &in, bool fill, uint32_t *d_cnt, const unsigned long long *d_ptr, int32_t *d_ends)
{
    return hw_for_words(c, [&](auto w) -> int {
        constexpr int W = decltype(w)::value;
        if (fill) hipLaunchKernelGGL((k_shw_ends<W, 1>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, d_ends);
        else hipLaunchKernelGGL((k_shw_ends<W, 0>), dim3((in.n_tiles + 3) / 4), dim3(256), 0, 0, st->dev, in, d_cnt, d_ptr, d_ends);
        ISO_HIP_CHECK(hipGetLastError());
        return ISOCON_OK;
    });
}

// What both entries share: the pair arrays in device memory, the driver and the distance stage.
struct ShwCall {
    isocon_store *s;
    const char *entry;
    ScratchPool *pl;
    HwDriver drv;
    DevBuf d_q, d_t, d_k, d_he, d_thr, d_enter;
    EventTimer tm;
    std::vector<int32_t> he;          // host copy of (h or -1, first end) per pair, after distances()
    ShwCall(isocon_store *st, const char *who)
        : s(st), entry(who), pl(&g_scratch), drv(st, pl), d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_thr(pl, SLOT_HWL_THR),
          d_enter(pl, SLOT_SHW_ENTER) {}

    int kernel_flags()
    {
        uint32_t flags = 0;
        ISO_HIP_CHECK(memcpy_wait(&flags, drv.flags(), 4, hipMemcpyDeviceToHost));
        return hw_flag_error(flags, entry, nullptr);
    }
    // STAGE 3 tiles over (d_q, d_t, d_thr); a tile band error cannot happen there
    int tiles(uint64_t n_pairs, HwStageTiles &tl)
    {
        int rc;
        if ((rc = drv.build_device<3>(n_pairs, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_thr.as<int32_t>(), nullptr, nullptr, tl)) ||
            (rc = hw_flag_error(tl.ctr.flags, entry, nullptr)))
            return rc;
        if (tl.ctr.flags & HWT_ERR_TILE_BAND) { g_last_error = std::string(entry) + ": internal status (tile band)"; return ISOCON_E_HIP; }
        return ISOCON_OK;
    }
    // he = (h or -1, first end) of every pair; ISOCON_E_UNSUPPORTED for a pair that no round settles
    int distances(const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs)
    {
        int rc;
        if ((rc = d_q.upload(q, n_pairs * 4)) || (rc = d_t.upload(t, n_pairs * 4)) || (rc = d_k.upload(k, n_pairs * 4)) || (rc = d_he.alloc(n_pairs * 8)) ||
            (rc = d_thr.alloc(n_pairs * 4)) || (rc = d_enter.alloc(SHW_ROUNDS * 4)) || (rc = drv.size(n_pairs)))
            return rc;
        ISO_HIP_CHECK(hipMemsetAsync(d_enter.p, 0, SHW_ROUNDS * 4, 0));
        const unsigned pb = (unsigned)((n_pairs + 255) / 256);
        tm.start();
        for (int r = 0; r < SHW_ROUNDS; ++r) {
            hipLaunchKernelGGL(k_shw_round, dim3(pb), dim3(256), 0, 0, s->dev, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_k.as<int32_t>(), (unsigned long long)n_pairs, r,
                               d_he.as<int32_t>(), d_thr.as<int32_t>(), d_enter.as<uint32_t>());
            ISO_HIP_CHECK(hipGetLastError());
            uint32_t enter[SHW_ROUNDS];
            ISO_HIP_CHECK(memcpy_wait(enter, d_enter.p, sizeof enter, hipMemcpyDeviceToHost));
            if (r > 0) {
                if ((rc = kernel_flags())) return rc;          // (of the round before: the builder zeroes the word)
                if (!enter[r]) break;
            }
            g_shw_stats[SW_ROUNDS] = r + 1;
            g_shw_stats[SW_ENTER + r] = (double)enter[r];
            HwStageTiles tl;
            if ((rc = tiles(n_pairs, tl))) return rc;
            double per_class[4] = {0, 0, 0, 0};
            if ((rc = drv.for_classes(tl, d_t.as<uint32_t>(), d_thr.as<int32_t>(), per_class,
                                      [&](int c, const HwTileIn &in) { return shw_launch_locate(s, c, in, d_he.as<int32_t>()); })))
                return rc;
            for (int c = 0; c < 4; ++c) g_shw_stats[SW_LOCATE + c] += per_class[c];
        }
        tm.stop();
        if ((rc = kernel_flags())) return rc;
        he.resize(n_pairs * 2);
        ISO_HIP_CHECK(copy_d2h(he.data(), d_he.p, n_pairs * 8));
        const std::vector<int32_t> &lens = s->lens;
        uint64_t hits = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            if (he[p * 2] >= 0) { ++hits; continue; }
            if (std::min(k[p], lens[q[p]]) > shw_round_thr(SHW_ROUNDS - 1)) {
                g_last_error = std::string(entry) + ": pair " + std::to_string(p) + " is above distance " + std::to_string(shw_round_thr(SHW_ROUNDS - 1)) +
                               " under a threshold beyond it (the prefix kernels hold 511 diagonals; not supported)";
                return ISOCON_E_UNSUPPORTED;
            }
        }
        g_shw_stats[SW_HITS] = (double)hits;
        return ISOCON_OK;
    }
};

int shw_check(isocon_store *s, uint64_t n_pairs)
{
    if (s->n_exc) { g_last_error = "prefix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    if (n_pairs > 0xfffffff0ull || (uint64_t)s->dev.n * 4 >= 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_shw_last_stats(double *out, int32_t cap) { return copy_last_stats(g_shw_stats, SW_COUNT, out, cap); }

extern "C" int isocon_shw_locations(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out_ed,
                                    uint64_t *out_end_ptr, int32_t *out_ends, uint64_t cap, uint64_t *needed, float *kernel_ms)
{
    for (double &x : g_shw_stats) x = 0;
    if (!s || !out_end_ptr || (n_pairs && (!q || !t || !k || !out_ed)) || (cap && !out_ends)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (needed) *needed = 0;
    out_end_ptr[0] = 0;
    if (!n_pairs) return ISOCON_OK;
    int rc;
    if ((rc = shw_check(s, n_pairs))) return rc;
    g_shw_stats[SW_PAIRS] = (double)n_pairs;
    HostClock clk;
    ShwCall call(s, "isocon_shw_locations");
    if ((rc = call.distances(q, t, k, n_pairs))) return rc;
    clk.lap("shw locations: distances");
    // ---- ENDS, first run: how many columns of every hit attain its distance ----
    ScratchPool *pl = call.pl;
    DevBuf d_cnt(pl, SLOT_HWL_CNT), d_ptr(pl, SLOT_HWL_PTR), d_ends(pl, SLOT_HWL_LOCS);
    if ((rc = d_cnt.alloc(n_pairs * 4)) || (rc = d_ptr.alloc((n_pairs + 1) * 8))) return rc;
    call.tm.start();
    hipLaunchKernelGGL(k_shw_prep, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, 0, call.d_he.as<int32_t>(), (unsigned long long)n_pairs,
                       call.d_thr.as<int32_t>(), d_cnt.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    HwStageTiles tl;
    if ((rc = call.tiles(n_pairs, tl))) return rc;
    auto ends = [&](bool fill) -> int {
        return call.drv.for_classes(tl, call.d_t.as<uint32_t>(), call.d_thr.as<int32_t>(), fill ? nullptr : g_shw_stats + SW_ENDS_TILES, [&](int c, const HwTileIn &in) {
            return shw_launch_ends(s, c, in, fill, d_cnt.as<uint32_t>(), d_ptr.as<unsigned long long>(), d_ends.as<int32_t>());
        });
    };
    if ((rc = ends(false))) return rc;
    if ((rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), (uint32_t)n_pairs, d_ptr.as<unsigned long long>()))) return rc;
    call.tm.stop();
    clk.lap("shw locations: ends (count), scan");
    if ((rc = call.kernel_flags())) return rc;
    // ---- the caller's distances and row pointers; the total sizes the list ----
    for (uint64_t p = 0; p < n_pairs; ++p) out_ed[p] = call.he[p * 2] >= 0 ? call.he[p * 2] : -1;
    ISO_HIP_CHECK(copy_d2h(out_end_ptr, d_ptr.p, (n_pairs + 1) * 8));
    const uint64_t total = out_end_ptr[n_pairs];
    g_shw_stats[SW_ENDS] = (double)total;
    if (needed) *needed = total;
    if (kernel_ms) *kernel_ms = call.tm.total;
    if (total > cap) return ISOCON_E_CAPACITY;
    if (!total) return ISOCON_OK;
    if (total > 0xfffffff0ull) { g_last_error = "isocon_shw_locations: more than 2^32 - 16 ends in one call"; return ISOCON_E_UNSUPPORTED; }
    // ---- ENDS, second run: every end into its slot ----
    if ((rc = d_ends.alloc(total * 4))) return rc;
    call.tm.start();
    if ((rc = ends(true))) return rc;
    call.tm.stop();
    clk.lap("shw locations: ends (fill)");
    if ((rc = call.kernel_flags())) return rc;
    ISO_HIP_CHECK(copy_d2h(out_ends, d_ends.p, total * 4));
    if (kernel_ms) *kernel_ms = call.tm.total;
    return ISOCON_OK;
}

extern "C" int isocon_shw_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out,
                                     uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms)
{
    for (double &x : g_shw_stats) x = 0;
    int rc;
    if (path_prologue(s, n_pairs, {q, t, k, out}, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms, &rc)) return rc;
    if ((rc = shw_check(s, n_pairs))) return rc;
    g_shw_stats[SW_PAIRS] = (double)n_pairs;
    HostClock clk;
    NwpHits H;
    {
        // ---- rows: distance and first end (the call's scratch is released before the path stage takes its own) ----
        ShwCall call(s, "isocon_shw_path_pairs");
        if ((rc = call.distances(q, t, k, n_pairs))) return rc;
        if (kernel_ms) *kernel_ms = call.tm.total;
        const std::vector<int32_t> &lens = s->lens;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const int32_t h = call.he[p * 2], end = call.he[p * 2 + 1];
            out[p * 2] = h >= 0 ? h : -1;
            out[p * 2 + 1] = h >= 0 ? end : -1;
            if (h < 0) continue;
            if (end < 0 || end >= lens[t[p]]) { g_last_error = "isocon_shw_path_pairs: internal status (end) for pair " + std::to_string(p); return ISOCON_E_HIP; }
            // the global alignment of the query against t[0 .. end]: h <= 255, so every hit takes the banded trace
            H.pair.push_back(p); H.q.push_back(q[p]); H.t.push_back(t[p]); H.ed.push_back(h);
            H.start.push_back(0); H.cols.push_back(end + 1);
        }
    }
    clk.lap("shw path: rows");
    return nwp_paths(s, "isocon_shw_path_pairs", "shw path", H, n_pairs, [](uint64_t) -> uint64_t { return 0; }, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms, clk);
}
