// nw_path_host.inc -- host side of isocon_ed_path_pairs (included by isocon_hip.hip after hw_full_host.inc): the bounded distances
// through the implementation of isocon_ed_pairs, then the paths of the pairs within their threshold through nw_band.hpp (the hits whose
// corridor fits 256 diagonals) and nw_path.hpp (the others).  nwp_paths, the driver of that second part, is shared with
// isocon_hw_path_pairs (hw_path_host.inc), whose hits are traced over a window.

namespace {

// Trace scratch one launch of k_nwp_trace may hold (SLOT_HW_TRACE, shared with the un-banded infix kernels): the host cuts the hits
// into as many launches as that takes, a pair whose own store exceeds it is refused.  ISOCON_DEBUG_VARIANT=nwp_trace_budget=<bytes>
// (tests: many launches at small shapes).  The LDS limit of the boundary row is kHwfMaxLds.
static constexpr uint64_t kNwpTraceBudget = (uint64_t)1 << 30;

// The same for one launch of k_nwb_trace (nw_band.hpp, SLOT_NWB_TRACE), counted on the regions of its waves: a hit whose corridor fits
// 256 diagonals is traced there, on 16 bytes per column and window word.  A wave whose region exceeds the budget is cut into waves of
// fewer lanes, a pair whose own columns exceed it is refused.  ISOCON_DEBUG_VARIANT=nwp_band_budget=<bytes> (tests).
// nwp_unbanded sends every hit through k_nwp_trace; nwp_trace_budget= implies it (whoever sets that budget means that store).
static constexpr uint64_t kNwpBandBudget = (uint64_t)1 << 30;

// isocon_path_last_stats: the calling thread's last path call.
enum { PS_HITS = 0, PS_W1, PS_W2, PS_W4, PS_UNBANDED, PS_BYTES_BAND, PS_BYTES_UNBANDED, PS_LAUNCHES_BAND, PS_LAUNCHES_UNBANDED, PS_MS_BAND, PS_MS_UNBANDED, PS_MS_EMIT,
       PS_COUNT };
thread_local double g_path_stats[PS_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// Both path entries call this first: a call that traces nothing, or fails before or while its hits are classed, reports zeros.
inline void path_stats_reset() { for (double &x : g_path_stats) x = 0; }

// 16-byte units of the region of a band wave: [column][word][lane], the columns rounded up to the blocks of 32 the kernel works in
inline int32_t nwb_region_cols(int32_t cols) { return (cols + 31) & ~31; }
inline uint64_t nwb_region_units(int32_t cols, int32_t W, int32_t lanes) { return (uint64_t)nwb_region_cols(cols) * (uint64_t)W * (uint64_t)lanes; }

template <int W>
void nwb_launch(bool window, unsigned waves, const DevStore &dev, const NwbIn &in, ulonglong2 *trace, uint32_t *rev, int32_t *runs)
{
    if (window) hipLaunchKernelGGL((k_nwb_trace<W, true>), dim3(waves), dim3(64), 0, 0, dev, in, trace, rev, runs);
    else hipLaunchKernelGGL((k_nwb_trace<W, false>), dim3(waves), dim3(64), 0, 0, dev, in, trace, rev, runs);
}

// The pairs whose path is traced, in the order of the list.  start / cols: the window of the target of each (isocon_hw_path_pairs);
// both empty: the whole target (isocon_ed_path_pairs).
struct NwpHits {
    std::vector<uint64_t> pair;
    std::vector<uint32_t> q, t;
    std::vector<int32_t> ed, start, cols;
    bool window() const { return !start.empty() || !cols.empty(); }
};

// What both path entries do once the distances (and windows) are known: the class of every hit, trace store and slice of reversed runs of
// each, the launches of k_nwb_trace and k_nwp_trace cut by their budgets, out_ops_ptr, the capacity protocol and k_nwp_emit into out_ops.
// extra(p): the ops a pair that is no hit owns (the caller writes them after ISOCON_OK).  *kernel_ms gains the time of the launches.
template <class Extra>
int nwp_paths(isocon_store *s, const char *who, const char *lap, const NwpHits &H, uint64_t n_pairs, Extra extra, uint32_t *out_ops, uint64_t *out_ops_ptr,
              uint64_t ops_cap, uint64_t *needed, float *kernel_ms, HostClock &clk)
{
    const std::vector<int32_t> &lens = s->lens;
    const bool window = H.window();
    const std::string name(who), stage(lap);
    const size_t nh = H.pair.size();
    int rc;
    path_stats_reset();
    uint64_t budget = kNwpTraceBudget, band_budget = kNwpBandBudget;
    bool unbanded = variant("nwp_unbanded");
    if (const char *e = variant_value("nwp_trace_budget")) { budget = strtoull(e, nullptr, 10); unbanded = true; }
    if (const char *e = variant_value("nwp_band_budget")) band_budget = strtoull(e, nullptr, 10);
    // ---- the class of every hit (0: un-banded) and what its store needs ----
    std::vector<int32_t> cls(nh, 0), ncols(nh, 0);
    std::vector<uint64_t> units_of(nh, 0);
    size_t lds = 0, nu = 0;
    double per_class[5] = {0, 0, 0, 0, 0};          // by W; into the stats once no hit has been refused
    for (size_t i = 0; i < nh; ++i) {
        const int32_t m = lens[H.q[i]], nt = lens[H.t[i]], nc = window ? H.cols[i] : nt;
        if (window && (H.start[i] < 0 || nc <= 0 || nc > nt - H.start[i])) {
            g_last_error = name + ": internal status (window) for pair " + std::to_string(H.pair[i]);
            return ISOCON_E_HIP;
        }
        ncols[i] = nc;
        if (!unbanded && m > 0 && nc > 0 && H.ed[i] >= 0) cls[i] = nwb_class(m - nc, H.ed[i]);
        const std::string sizes = "a query of " + std::to_string(m) + " bases against a target of " + std::to_string(nt) + " bases" +
                                  (window ? " (window of " + std::to_string(nc) + " columns)" : std::string());
        if (cls[i]) {
            const uint64_t need = nwb_region_units(nc, cls[i], 1) * 16;
            if (need > band_budget) {
                g_last_error = name + ": the banded trace of " + sizes + " needs " + std::to_string(need) + " bytes (budget " + std::to_string(band_budget) + ")";
                return ISOCON_E_UNSUPPORTED;
            }
            per_class[cls[i]] += 1;
            continue;
        }
        const uint64_t u = hwf_trace_units(m, nc);
        if (u * 16 > budget) {
            g_last_error = name + ": the trace of " + sizes + " needs " + std::to_string(u * 16) + " bytes (budget " + std::to_string(budget) + ")";
            return ISOCON_E_UNSUPPORTED;
        }
        if (hwf_passes(m) > 1) lds = std::max(lds, (size_t)hwf_bound_words(nc) * 4);
        units_of[i] = u;
        ++nu;
    }
    if (lds > kHwfMaxLds) {
        g_last_error = name + ": a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
        return ISOCON_E_UNSUPPORTED;
    }
    g_path_stats[PS_HITS] = (double)nh; g_path_stats[PS_UNBANDED] = (double)nu;
    g_path_stats[PS_W1] = per_class[1]; g_path_stats[PS_W2] = per_class[2]; g_path_stats[PS_W4] = per_class[4];
    // ---- the order on the device: the un-banded hits in the order of the list, then the band hits by class and by number of columns (a
    //      wave's region is sized by its longest lane).  Whatever is indexed "by position" below follows it; ord[position] = hit ----
    std::vector<uint32_t> ord(nh);
    {
        size_t a = 0, b = nu;
        for (size_t i = 0; i < nh; ++i) ord[cls[i] ? b++ : a++] = (uint32_t)i;
        std::sort(ord.begin() + nu, ord.end(), [&](uint32_t x, uint32_t y) {
            return cls[x] != cls[y] ? cls[x] < cls[y] : ncols[x] != ncols[y] ? ncols[x] < ncols[y] : x < y;
        });
    }
    std::vector<uint32_t> pq(nh), pt(nh);
    std::vector<int32_t> ped(nh), pstart(nh, 0), pcols(nh), pcls(nh);
    std::vector<uint64_t> units(nh), rev_off(nh);
    uint64_t rev_total = 0;
    for (size_t p = 0; p < nh; ++p) {
        const uint32_t i = ord[p];
        pq[p] = H.q[i]; pt[p] = H.t[i]; ped[p] = H.ed[i]; pcols[p] = ncols[i]; pcls[p] = cls[i]; units[p] = units_of[i];
        if (window) pstart[p] = H.start[i];
        rev_off[p] = rev_total;
        rev_total += nwp_max_runs(H.ed[i]);
    }
    std::vector<int32_t> runs(nh, 0);          // by hit
    EventTimer tm, tm_band, tm_emit;
    ScratchPool *pl = &s->pool;
    DevBuf d_q(pl, SLOT_NWP_Q), d_t(pl, SLOT_NWP_T), d_ed(pl, SLOT_NWP_ED), d_toff(pl, SLOT_NWP_TOFF), d_roff(pl, SLOT_NWP_ROFF), d_rev(pl, SLOT_NWP_REV),
        d_runs(pl, SLOT_NWP_RUNS), d_foff(pl, SLOT_NWP_FOFF), d_ops(pl, SLOT_NWP_OPS), d_trace(pl, SLOT_HW_TRACE), d_start(pl, SLOT_NWP_START),
        d_cols(pl, SLOT_NWP_COLS), d_btrace(pl, SLOT_NWB_TRACE), d_slots(pl, SLOT_NWB_SLOTS), d_woff(pl, SLOT_NWB_WOFF), d_wcols(pl, SLOT_NWB_WCOLS),
        d_wlanes(pl, SLOT_NWB_WLANES);
    size_t launches = 0, band_launches = 0;
    uint64_t trace_bytes = 0, band_bytes = 0;
    if (nh) {
        if ((rc = d_q.alloc(nh * 4)) || (rc = d_t.alloc(nh * 4)) || (rc = d_ed.alloc(nh * 4)) || (rc = d_roff.alloc(nh * 8)) ||
            (rc = d_rev.alloc((size_t)rev_total * 4)) || (rc = d_runs.alloc(nh * 4)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_q.p, pq.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_t.p, pt.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_ed.p, ped.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_roff.p, rev_off.data(), nh * 8));
        if (window) {
            if ((rc = d_start.alloc(nh * 4)) || (rc = d_cols.alloc(nh * 4))) return rc;
            ISO_HIP_CHECK(copy_h2d(d_start.p, pstart.data(), nh * 4));
            ISO_HIP_CHECK(copy_h2d(d_cols.p, pcols.data(), nh * 4));
        }
    }
    if (nu) {
        // the un-banded launches (positions 0 .. nu - 1): consecutive hits whose stores fit the budget together; trace_off is relative to its launch
        std::vector<uint64_t> toff(nu);
        std::vector<size_t> cut(1, 0);
        uint64_t total = 0, most = 0;
        for (size_t i = 0; i < nu; ++i) {
            if ((total + units[i]) * 16 > budget || i - cut.back() >= ((size_t)1 << 20)) { cut.push_back(i); total = 0; }
            toff[i] = total; total += units[i];
            most = std::max(most, total);
            trace_bytes += units[i] * 16;
        }
        cut.push_back(nu);
        if ((rc = d_toff.alloc(nu * 8)) || (rc = d_trace.alloc((size_t)most * 16))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_toff.p, toff.data(), nu * 8));
        const void *kern = window ? (const void *)k_nwp_trace<true> : (const void *)k_nwp_trace<false>;
        if (lds > ((size_t)64 << 10)) ISO_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            const size_t a = cut[c], cnt = cut[c + 1] - a;
            NwpIn in{};
            in.pq = d_q.as<uint32_t>() + a; in.pt = d_t.as<uint32_t>() + a; in.ed = d_ed.as<int32_t>() + a;
            in.trace_off = d_toff.as<uint64_t>() + a; in.rev_off = d_roff.as<uint64_t>() + a; in.n = (uint32_t)cnt;
            tm.start();
            if (window) {
                in.t_start = d_start.as<int32_t>() + a; in.t_cols = d_cols.as<int32_t>() + a;
                hipLaunchKernelGGL(k_nwp_trace<true>, dim3((unsigned)cnt), dim3(64), lds, 0, s->dev, in, d_trace.as<ulonglong2>(), d_rev.as<uint32_t>(),
                                   d_runs.as<int32_t>() + a);
            } else {
                hipLaunchKernelGGL(k_nwp_trace<false>, dim3((unsigned)cnt), dim3(64), lds, 0, s->dev, in, d_trace.as<ulonglong2>(), d_rev.as<uint32_t>(),
                                   d_runs.as<int32_t>() + a);
            }
            ISO_HIP_CHECK(hipGetLastError());
            tm.stop();                                      // also the fence before the next launch reuses the store
            ++launches;
        }
    }
    if (nh > nu) {
        // the band waves (positions nu .. nh - 1): up to 64 consecutive positions of one class, the last of them the longest; a region above
        // the budget is cut into waves of fewer lanes (every pair fits alone: checked above)
        struct Wave { size_t first; int32_t cnt, W, cols, lanes; uint64_t units; };
        std::vector<Wave> waves;
        for (size_t p = nu; p < nh;) {
            const int32_t W = pcls[p];
            size_t e = p;
            while (e < nh && e - p < 64 && pcls[e] == W) ++e;
            if (nwb_region_units(pcols[e - 1], W, (int32_t)(e - p)) * 16 > band_budget) {
                const uint64_t per = std::max<uint64_t>(1, band_budget / (nwb_region_units(pcols[e - 1], W, 1) * 16));
                e = p + (size_t)std::min<uint64_t>(per, e - p);
            }
            const int32_t lanes = (int32_t)(e - p);          // a region has the lanes of its wave: 64 but for the last wave of a class
            waves.push_back(Wave{p, (int32_t)(e - p), W, nwb_region_cols(pcols[e - 1]), lanes, nwb_region_units(pcols[e - 1], W, lanes)});
            p = e;
        }
        const size_t nw = waves.size();
        std::vector<uint32_t> slots(nw * 64, 0xffffffffu);
        std::vector<uint64_t> woff(nw);
        std::vector<int32_t> wcols(nw), wlanes(nw);
        std::vector<size_t> cut(1, 0);
        uint64_t total = 0, most = 0;
        for (size_t w = 0; w < nw; ++w) {
            const Wave &v = waves[w];
            for (int32_t l = 0; l < v.cnt; ++l) slots[w * 64 + l] = (uint32_t)(v.first + l);
            wcols[w] = v.cols; wlanes[w] = v.lanes;
            if (w > cut.back() && ((total + v.units) * 16 > band_budget || v.W != waves[w - 1].W || w - cut.back() >= ((size_t)1 << 20))) { cut.push_back(w); total = 0; }
            woff[w] = total; total += v.units;
            most = std::max(most, total);
            band_bytes += v.units * 16;
        }
        cut.push_back(nw);
        if ((rc = d_slots.alloc(nw * 64 * 4)) || (rc = d_woff.alloc(nw * 8)) || (rc = d_wcols.alloc(nw * 4)) || (rc = d_wlanes.alloc(nw * 4)) ||
            (rc = d_btrace.alloc((size_t)most * 16)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_slots.p, slots.data(), nw * 64 * 4));
        ISO_HIP_CHECK(copy_h2d(d_woff.p, woff.data(), nw * 8));
        ISO_HIP_CHECK(copy_h2d(d_wcols.p, wcols.data(), nw * 4));
        ISO_HIP_CHECK(copy_h2d(d_wlanes.p, wlanes.data(), nw * 4));
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            const size_t a = cut[c], cnt = cut[c + 1] - a;
            NwbIn in{};
            in.slot_hit = d_slots.as<uint32_t>() + a * 64; in.wave_off = d_woff.as<uint64_t>() + a; in.wave_cols = d_wcols.as<int32_t>() + a;
            in.wave_lanes = d_wlanes.as<int32_t>() + a;
            in.pq = d_q.as<uint32_t>(); in.pt = d_t.as<uint32_t>(); in.ed = d_ed.as<int32_t>(); in.rev_off = d_roff.as<uint64_t>();
            in.t_start = window ? d_start.as<int32_t>() : nullptr; in.t_cols = window ? d_cols.as<int32_t>() : nullptr;
            in.n_waves = (uint32_t)cnt;
            tm_band.start();
            const int32_t W = waves[a].W;
            if (W == 1) nwb_launch<1>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            else if (W == 2) nwb_launch<2>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            else nwb_launch<4>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            ISO_HIP_CHECK(hipGetLastError());
            tm_band.stop();                                 // also the fence before the next launch reuses the store
            ++band_launches;
        }
    }
    if (nh) {
        std::vector<int32_t> got(nh);
        ISO_HIP_CHECK(copy_d2h(got.data(), d_runs.p, nh * 4));
        for (size_t p = 0; p < nh; ++p) {
            if (got[p] <= 0 || (uint64_t)got[p] > nwp_max_runs(ped[p])) {
                g_last_error = name + ": internal status " + std::to_string(got[p]) + " for pair " + std::to_string(H.pair[ord[p]]);
                return ISOCON_E_HIP;
            }
            runs[ord[p]] = got[p];
        }
    }
    g_path_stats[PS_BYTES_BAND] = (double)band_bytes; g_path_stats[PS_BYTES_UNBANDED] = (double)trace_bytes;
    g_path_stats[PS_LAUNCHES_BAND] = (double)band_launches; g_path_stats[PS_LAUNCHES_UNBANDED] = (double)launches;
    g_path_stats[PS_MS_BAND] = tm_band.total; g_path_stats[PS_MS_UNBANDED] = tm.total;
    if (clk.on)
        fprintf(stderr, "[isocon] %s: %llu pairs, %zu traced (%zu un-banded), %zu + %zu launches, %llu + %llu bytes of trace\n", lap, (unsigned long long)n_pairs, nh, nu,
                band_launches, launches, (unsigned long long)band_bytes, (unsigned long long)trace_bytes);
    clk.lap((stage + ": trace + walk").c_str());
    // ---- offsets of the dense forward list: a traced pair has its runs, another pair what the caller says ----
    {
        size_t h = 0;
        uint64_t at = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            out_ops_ptr[p] = at;
            if (h < nh && H.pair[h] == p) at += (uint64_t)runs[h++];
            else at += extra(p);
        }
        out_ops_ptr[n_pairs] = at;
    }
    const uint64_t total_ops = out_ops_ptr[n_pairs];
    if (needed) *needed = total_ops;
    if (total_ops > ops_cap) {
        if (kernel_ms) *kernel_ms += tm.total + tm_band.total;
        g_last_error = name + ": " + std::to_string(total_ops) + " ops, room for " + std::to_string(ops_cap);
        return ISOCON_E_CAPACITY;
    }
    if (nh) {
        std::vector<uint64_t> foff(nh);          // by position, like the reversed runs
        for (size_t p = 0; p < nh; ++p) foff[p] = out_ops_ptr[H.pair[ord[p]]];
        if ((rc = d_foff.alloc(nh * 8)) || (rc = d_ops.alloc((size_t)total_ops * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_foff.p, foff.data(), nh * 8));
        tm_emit.start();
        hipLaunchKernelGGL(k_nwp_emit, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, 0, d_rev.as<uint32_t>(), d_roff.as<uint64_t>(), d_runs.as<int32_t>(),
                           d_foff.as<uint64_t>(), (uint32_t)nh, d_ops.as<uint32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm_emit.stop();
        ISO_HIP_CHECK(copy_d2h(out_ops, d_ops.p, (size_t)total_ops * 4));
    }
    g_path_stats[PS_MS_EMIT] = tm_emit.total;
    if (kernel_ms) *kernel_ms += tm.total + tm_band.total + tm_emit.total;
    clk.lap((stage + ": forward ops").c_str());
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_path_last_stats(double *out, int32_t cap)
{
    if (!out || cap < 0) return 0;
    const int k = cap < (int)PS_COUNT ? cap : (int)PS_COUNT;
    for (int i = 0; i < k; ++i) out[i] = g_path_stats[i];
    return k;
}

extern "C" int isocon_ed_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                                    int32_t *out_ed, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms)
{
    path_stats_reset();
    if (!s || !out_ops_ptr || (n_pairs && (!q || !t || !out_ed)) || (ops_cap && !out_ops)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (needed) *needed = 0;
    out_ops_ptr[0] = 0;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "alignment paths run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    if (n_pairs > 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    const uint32_t n = s->dev.n;
    const std::vector<int32_t> &lens = s->lens;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (q[p] >= n || t[p] >= n) { g_last_error = "pair index out of range"; return ISOCON_E_ARG; }
    HostClock clk;
    // ---- distances: pairs with an empty sequence on the host, the others as one call of isocon_ed_pairs' implementation ----
    std::vector<uint64_t> full;          // pairs of two non-empty sequences
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const int32_t m = lens[q[p]], nt = lens[t[p]];
        if (m > 0 && nt > 0) { full.push_back(p); continue; }
        const int32_t d = m > nt ? m : nt, kk = k ? k[p] : -1;
        out_ed[p] = kk >= 0 && d > kk ? -1 : d;
    }
    float ms_ed = 0.f;
    int rc;
    if (!full.empty()) {
        const size_t nf = full.size();
        std::vector<uint32_t> fq(nf), ft(nf);
        std::vector<int32_t> fk(nf), fe(nf, -1);
        for (size_t i = 0; i < nf; ++i) { fq[i] = q[full[i]]; ft[i] = t[full[i]]; fk[i] = k ? k[full[i]] : -1; }
        if ((rc = ed_pairs_impl(s, fq.data(), ft.data(), fk.data(), nf, fe.data(), &ms_ed, nullptr, false))) return rc;
        for (size_t i = 0; i < nf; ++i) out_ed[full[i]] = fe[i] < 0 ? -1 : fe[i];
    }
    clk.lap("ed path: distances");
    // ---- the hits, then what both path entries share ----
    NwpHits H;
    for (uint64_t p : full) {
        if (out_ed[p] < 0) continue;
        H.pair.push_back(p); H.q.push_back(q[p]); H.t.push_back(t[p]); H.ed.push_back(out_ed[p]);
    }
    // a hit with one empty sequence is one op (none if both are)
    auto extra = [&](uint64_t p) -> uint64_t { return out_ed[p] > 0 && (lens[q[p]] == 0 || lens[t[p]] == 0) ? 1 : 0; };
    if (kernel_ms) *kernel_ms = ms_ed;
    if ((rc = nwp_paths(s, "isocon_ed_path_pairs", "ed path", H, n_pairs, extra, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms, clk))) return rc;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const int32_t m = lens[q[p]], nt = lens[t[p]];
        if (out_ed[p] > 0 && (m == 0 || nt == 0)) out_ops[out_ops_ptr[p]] = m == 0 ? nwp_op(NWP_D, nt) : nwp_op(NWP_I, m);
    }
    return ISOCON_OK;
}
