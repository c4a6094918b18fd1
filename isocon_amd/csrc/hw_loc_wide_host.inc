// hw_loc_wide_host.inc -- host side of isocon_hw_locations_wide (included by isocon_hip.hip after hw_loc_host.inc and hw_full_host.inc):
// the pairs whose own band fits the 512 diagonals of hw.hpp go through isocon_hw_locations as one sub-list, the others through the
// kernels of hw_rows.hpp -- count run, scan, fill run, then the START of every (pair, end) entry -- and the two CSR results are merged
// into the caller's order.  The wide part keeps scratch slots of its own: the banded call runs between its two halves.

namespace {

// isocon_hw_locations_wide_last_stats
enum {
    HLW_PAIRS = 0, HLW_NARROW, HLW_WIDE, HLW_HITS, HLW_LOCATIONS, HLW_ROWS_W1, HLW_ROWS_W2, HLW_ROWS_W4, HLW_WAVE, HLW_START_BANDED, HLW_START_FULL,
    HLW_LAUNCHES, HLW_KERNEL_MS, HLW_COUNT
};
thread_local double g_hwlw_stats[HLW_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// queries of at most this many rows take the lane-per-pair kernel (DESIGN.md 4.7: measured); ISOCON_DEBUG_VARIANT=hwl_rows_max=<rows>
static constexpr int32_t kHwlRowsMax = 256;

// The wide pairs of one call: count() leaves h, the first end and the row pointers of the wide list on the host (and everything the fill
// needs on the device), fill() the (start, end) rows.
struct HwlWide {
    isocon_store *s;
    ScratchPool *pl = &g_scratch;
    size_t nw = 0, lds = 0;
    DevBuf d_q, d_t, d_k, d_he, d_cnt, d_ptr, d_list, d_flags;
    std::vector<uint32_t> cls[4];          // the pairs of W = 1, 2, 4 and of the wavefront kernel
    size_t cls_at[4] = {0, 0, 0, 0};
    std::vector<int32_t> he;
    std::vector<uint64_t> ptr;
    EventTimer tm;
    explicit HwlWide(isocon_store *st)
        : s(st), d_q(pl, SLOT_HWLW_Q), d_t(pl, SLOT_HWLW_T), d_k(pl, SLOT_HWLW_K), d_he(pl, SLOT_HWLW_HE), d_cnt(pl, SLOT_HWLW_CNT), d_ptr(pl, SLOT_HWLW_PTR),
          d_list(pl, SLOT_HWLW_LIST), d_flags(pl, SLOT_HWLW_FLAGS) {}

    HwlIn input(int c)
    {
        HwlIn in{};
        in.pq = d_q.as<uint32_t>(); in.pt = d_t.as<uint32_t>(); in.pk = d_k.as<int32_t>();
        in.list = d_list.as<uint32_t>() + cls_at[c]; in.n = (uint32_t)cls[c].size();
        in.he = d_he.as<int32_t>(); in.cnt = d_cnt.as<uint32_t>(); in.loc_ptr = d_ptr.as<unsigned long long>(); in.flags = d_flags.as<uint32_t>();
        return in;
    }
    template <int FILL>
    int run(const HwLocList &E)
    {
        for (int c = 0; c < 4; ++c) {
            if (cls[c].empty()) continue;
            const HwlIn in = input(c);
            const dim3 grid((in.n + kHwlRowsBlock - 1) / kHwlRowsBlock), block(kHwlRowsBlock);
            if (c == 0) hipLaunchKernelGGL((k_hwl_rows<1, FILL>), grid, block, 0, 0, s->dev, in, E);
            else if (c == 1) hipLaunchKernelGGL((k_hwl_rows<2, FILL>), grid, block, 0, 0, s->dev, in, E);
            else if (c == 2) hipLaunchKernelGGL((k_hwl_rows<4, FILL>), grid, block, 0, 0, s->dev, in, E);
            else hipLaunchKernelGGL((k_hwl_wave<FILL>), dim3(std::min<uint32_t>(in.n, 1u << 20)), dim3(64), lds, 0, s->dev, in, E);
            ISO_HIP_CHECK(hipGetLastError());
            g_hwlw_stats[HLW_LAUNCHES] += 1;
        }
        return ISOCON_OK;
    }
    int kernel_flags()
    {
        uint32_t flags = 0;
        ISO_HIP_CHECK(memcpy_wait(&flags, d_flags.p, 4, hipMemcpyDeviceToHost));
        if (flags) { g_last_error = "isocon_hw_locations_wide: internal status from a kernel"; return ISOCON_E_HIP; }
        return ISOCON_OK;
    }

    int count(const std::vector<uint32_t> &q, const std::vector<uint32_t> &t, const std::vector<int32_t> &k)
    {
        nw = q.size();
        const std::vector<int32_t> &lens = s->lens;
        int32_t rows_max = kHwlRowsMax;
        if (const char *e = variant_value("hwl_rows_max")) rows_max = std::max(64, std::min(256, atoi(e)));
        for (size_t x = 0; x < nw; ++x) {
            const int32_t m = lens[q[x]];
            const int w = m <= rows_max ? hwr_words(m) : 0;
            cls[w == 1 ? 0 : (w == 2 ? 1 : (w == 4 ? 2 : 3))].push_back((uint32_t)x);
            if (hwf_passes(m) > 1) lds = std::max(lds, (size_t)hwf_bound_words(lens[t[x]]) * 4);
        }
        if (lds > kHwfMaxLds) {
            g_last_error = "isocon_hw_locations_wide: a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
            return ISOCON_E_UNSUPPORTED;
        }
        for (int c = 0; c < 4; ++c) g_hwlw_stats[HLW_ROWS_W1 + c] = (double)cls[c].size();
        std::vector<uint32_t> list;
        list.reserve(nw);
        for (int c = 0; c < 4; ++c) { cls_at[c] = list.size(); list.insert(list.end(), cls[c].begin(), cls[c].end()); }
        int rc;
        if ((rc = d_q.upload(q.data(), nw * 4)) || (rc = d_t.upload(t.data(), nw * 4)) || (rc = d_k.upload(k.data(), nw * 4)) || (rc = d_list.upload(list.data(), nw * 4)) ||
            (rc = d_he.alloc(nw * 8)) || (rc = d_cnt.alloc(nw * 4)) || (rc = d_ptr.alloc((nw + 1) * 8)) || (rc = d_flags.alloc(4)))
            return rc;
        ISO_HIP_CHECK(hipMemsetAsync(d_flags.p, 0, 4, 0));
        if (lds > ((size_t)64 << 10)) {
            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_hwl_wave<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_hwl_wave<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_hwl_starts_full, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        tm.start();
        if (!(rc = run<0>(HwLocList{}))) rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), (uint32_t)nw, d_ptr.as<unsigned long long>());
        tm.stop();          // (on every path: the interval is closed before an error goes up)
        if (rc) return rc;
        he.resize(nw * 2);
        ptr.resize(nw + 1);
        ISO_HIP_CHECK(copy_d2h(he.data(), d_he.p, nw * 8));
        ISO_HIP_CHECK(copy_d2h(ptr.data(), d_ptr.p, (nw + 1) * 8));
        return ISOCON_OK;
    }

    // locs: ptr[nw] rows of (start, end) on the host
    int fill(int32_t *locs)
    {
        const uint64_t total = ptr[nw];
        if (!total) return ISOCON_OK;
        if (total > 0xfffffff0ull) { g_last_error = "isocon_hw_locations_wide: more than 2^32 - 16 locations in one call"; return ISOCON_E_UNSUPPORTED; }
        DevBuf d_eq(pl, SLOT_HWL_EQ), d_et(pl, SLOT_HWL_ET), d_eh(pl, SLOT_HWL_EH), d_ehe(pl, SLOT_HWL_EHE), d_locs(pl, SLOT_HWL_LOCS), d_ulist(pl, SLOT_HWLW_ULIST);
        int rc;
        if ((rc = d_eq.alloc(total * 4)) || (rc = d_et.alloc(total * 4)) || (rc = d_eh.alloc(total * 4)) || (rc = d_ehe.alloc(total * 8)) || (rc = d_locs.alloc(total * 8)))
            return rc;
        HwLocList E{};
        E.q = d_eq.as<uint32_t>(); E.t = d_et.as<uint32_t>(); E.h = d_eh.as<int32_t>(); E.he = d_ehe.as<int32_t>();
        // the entries by pair: h is the pair's, and a pair's entries are contiguous
        std::vector<uint32_t> ulist;
        uint64_t banded = 0;
        for (size_t x = 0; x < nw; ++x) {
            if (he[x * 2] <= kHwlBandedStartMax) { banded += ptr[x + 1] - ptr[x]; continue; }
            for (uint64_t e = ptr[x]; e < ptr[x + 1]; ++e) ulist.push_back((uint32_t)e);
        }
        g_hwlw_stats[HLW_START_BANDED] = (double)banded;
        g_hwlw_stats[HLW_START_FULL] = (double)ulist.size();
        if (!ulist.empty() && (rc = d_ulist.upload(ulist.data(), ulist.size() * 4))) return rc;
        const char *const entry = "isocon_hw_locations_wide";
        HwDriver drv(s, pl);
        if (banded && (rc = drv.size(total))) return rc;
        auto launches = [&]() -> int {
            int r;
            if ((r = run<1>(E))) return r;
            if (!ulist.empty()) {
                hipLaunchKernelGGL(k_hwl_starts_full, dim3(std::min<uint32_t>((uint32_t)ulist.size(), 1u << 20)), dim3(64), lds, 0, s->dev, E, d_ulist.as<uint32_t>(),
                                   (uint32_t)ulist.size(), d_locs.as<int32_t>(), d_flags.as<uint32_t>());
                ISO_HIP_CHECK(hipGetLastError());
                g_hwlw_stats[HLW_LAUNCHES] += 1;
            }
            if (!banded) return ISOCON_OK;
            // tiles by (query, class of 2 h + 1) on the expanded list, as isocon_hw_locations: the builder passes the entries of he = -1 by
            HwStageTiles ts;
            if ((r = drv.build_device<1>(total, E.q, E.t, E.h, E.he, nullptr, ts)) || (r = hw_flag_error(ts.ctr.flags, entry, nullptr))) return r;
            if (ts.ctr.flags & HWT_ERR_TILE_BAND) { g_last_error = "isocon_hw_locations_wide: internal status (tile band)"; return ISOCON_E_HIP; }
            double tiles[4];
            return drv.for_classes(ts, E.t, E.h, tiles, [&](int c, const HwTileIn &in) {
                g_hwlw_stats[HLW_LAUNCHES] += 1;
                return hw_launch_starts(s, c, in, E.he, d_locs.as<int32_t>());
            });
        };
        tm.start();
        rc = launches();
        tm.stop();          // (on every path: the interval is closed before an error goes up)
        if (rc) return rc;
        if (banded) {
            uint32_t flags = 0;
            ISO_HIP_CHECK(memcpy_wait(&flags, drv.flags(), 4, hipMemcpyDeviceToHost));
            if ((rc = hw_flag_error(flags, entry, nullptr))) return rc;
        }
        if ((rc = kernel_flags())) return rc;
        ISO_HIP_CHECK(copy_d2h(locs, d_locs.p, total * 8));
        return ISOCON_OK;
    }
};

}  // namespace

extern "C" int isocon_hw_locations_wide_last_stats(double *out, int32_t cap) { return copy_last_stats(g_hwlw_stats, HLW_COUNT, out, cap); }

extern "C" int isocon_hw_locations_wide(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs, int32_t *out_ed,
                                        uint64_t *out_loc_ptr, int32_t *out_locs, uint64_t cap, uint64_t *needed, float *kernel_ms)
{
    for (double &x : g_hwlw_stats) x = 0;
    if (!s || !out_loc_ptr || (n_pairs && (!q || !t || !k || !out_ed)) || (cap && !out_locs)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (needed) *needed = 0;
    out_loc_ptr[0] = 0;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    if (n_pairs > 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    const uint32_t n = s->dev.n;
    const std::vector<int32_t> &lens = s->lens;
    std::vector<uint64_t> wide;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (q[p] >= n || t[p] >= n) return ISOCON_E_ARG;
        if (k[p] < 0) { g_last_error = "isocon_hw_locations_wide: k must be >= 0"; return ISOCON_E_ARG; }
        if (k[p] > (1 << 20)) return ISOCON_E_UNSUPPORTED;
        if (!hwf_is_narrow(lens[q[p]], lens[t[p]], k[p])) wide.push_back(p);
    }
    g_hwlw_stats[HLW_PAIRS] = (double)n_pairs;
    g_hwlw_stats[HLW_NARROW] = (double)(n_pairs - wide.size());
    g_hwlw_stats[HLW_WIDE] = (double)wide.size();
    auto narrow_stats = [&](float ms) {
        g_hwlw_stats[HLW_HITS] += g_hw_loc_stats[HL_HITS];
        g_hwlw_stats[HLW_LOCATIONS] += g_hw_loc_stats[HL_LOCATIONS];
        g_hwlw_stats[HLW_KERNEL_MS] += ms;
    };
    if (wide.empty()) {
        float ms = 0.f;
        const int rc = isocon_hw_locations(s, q, t, k, n_pairs, out_ed, out_loc_ptr, out_locs, cap, needed, &ms);
        narrow_stats(ms);
        if (kernel_ms) *kernel_ms = ms;
        return rc;
    }
    int rc;
    // ---- the wide pairs: distance, first end and the number of ends ----
    const size_t nw = wide.size();
    HwlWide W(s);
    {
        std::vector<uint32_t> wq(nw), wt(nw);
        std::vector<int32_t> wk(nw);
        for (size_t i = 0; i < nw; ++i) { wq[i] = q[wide[i]]; wt[i] = t[wide[i]]; wk[i] = k[wide[i]]; }
        if ((rc = W.count(wq, wt, wk))) return rc;
    }
    const uint64_t total_wide = W.ptr[nw];
    // ---- the narrow pairs, in their order, as one call of the banded implementation (again with the room it asks for when the first
    //      guess is too small and the caller's capacity is not) ----
    const uint64_t n_narrow = n_pairs - nw;
    std::vector<int32_t> ned(n_narrow), nlocs;
    std::vector<uint64_t> nptr(n_narrow + 1, 0), at(n_narrow);
    uint64_t total_narrow = 0;
    float ms_narrow = 0.f;
    if (n_narrow) {
        std::vector<uint32_t> nq(n_narrow), nt(n_narrow);
        std::vector<int32_t> nk(n_narrow);
        size_t w = 0, c = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            if (w < nw && wide[w] == p) { ++w; continue; }
            nq[c] = q[p]; nt[c] = t[p]; nk[c] = k[p]; at[c] = p; ++c;
        }
        // The banded call gets no more room than the caller's buffer leaves behind the wide rows: with cap <= total_wide -- cap = 0, the
        // sizing call of the protocol -- it is asked with capacity 0 and stops behind its count run, and whenever it does fill its rows
        // (total_narrow <= ncap <= room) the combined total fits and the rows are used.
        const uint64_t room = cap > total_wide ? cap - total_wide : 0;
        uint64_t ncap =std::min<uint64_t>(room, std::max<uint64_t>(4 * n_narrow + 1024, 65536));
        for (;;) {
            nlocs.resize(ncap * 2);
            float ms = 0.f;
            rc = isocon_hw_locations(s, nq.data(), nt.data(), nk.data(), n_narrow, ned.data(), nptr.data(), nlocs.data(), ncap, &total_narrow, &ms);
            ms_narrow += ms;
            if (rc == ISOCON_E_CAPACITY && total_narrow <= room && ncap < total_narrow) { ncap = total_narrow; continue; }
            if (rc && rc != ISOCON_E_CAPACITY) return rc;
            break;
        }
        narrow_stats(ms_narrow);
    }
    // ---- distances and row pointers in the caller's order ----
    {
        size_t w = 0, c = 0;
        uint64_t at_loc = 0, hits = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            out_loc_ptr[p] = at_loc;
            if (w < nw && wide[w] == p) { out_ed[p] = W.he[w * 2]; at_loc += W.ptr[w + 1] - W.ptr[w]; hits += W.he[w * 2] >= 0; ++w; }
            else { out_ed[p] = ned[c]; at_loc += nptr[c + 1] - nptr[c]; ++c; }
        }
        out_loc_ptr[n_pairs] = at_loc;
        g_hwlw_stats[HLW_HITS] += (double)hits;
        g_hwlw_stats[HLW_LOCATIONS] += (double)total_wide;
    }
    const uint64_t total = total_wide + total_narrow;
    if (needed) *needed = total;
    g_hwlw_stats[HLW_KERNEL_MS] += W.tm.total;
    if (kernel_ms) *kernel_ms = ms_narrow + W.tm.total;
    if (total > cap) return ISOCON_E_CAPACITY;
    if (!total) return ISOCON_OK;
    // ---- the wide pairs' rows, then both parts into the caller's order ----
    std::vector<int32_t> wlocs(total_wide * 2);
    const float before = W.tm.total;
    if ((rc = W.fill(wlocs.data()))) return rc;
    g_hwlw_stats[HLW_KERNEL_MS] += W.tm.total - before;
    if (kernel_ms) *kernel_ms = ms_narrow + W.tm.total;
    size_t w = 0, c = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint64_t cnt = out_loc_ptr[p + 1] - out_loc_ptr[p];
        const bool is_wide = w < nw && wide[w] == p;
        const int32_t *src = is_wide ? wlocs.data() + W.ptr[w] * 2 : nlocs.data() + nptr[c] * 2;
        if (cnt) memcpy(out_locs + out_loc_ptr[p] * 2, src, cnt * 8);
        if (is_wide) ++w; else ++c;
    }
    return ISOCON_OK;
}
