// nw_path_host.inc -- host side of isocon_ed_path_pairs (included by isocon_hip.hip after hw_full_host.inc): the bounded distances
// through the implementation of isocon_ed_pairs, then the paths of the pairs within their threshold through nw_path.hpp.  nwp_paths,
// the driver of that second part, is shared with isocon_hw_path_pairs (hw_path_host.inc), whose hits are traced over a window.

namespace {

// Trace scratch one launch of k_nwp_trace may hold (SLOT_HW_TRACE, shared with the un-banded infix kernels): the host cuts the hits
// into as many launches as that takes, a pair whose own store exceeds it is refused.  ISOCON_DEBUG_VARIANT=nwp_trace_budget=<bytes>
// (tests: many launches at small shapes).  The LDS limit of the boundary row is kHwfMaxLds.
static constexpr uint64_t kNwpTraceBudget = (uint64_t)1 << 30;

// The pairs whose path is traced, in the order of the list.  start / cols: the window of the target of each (isocon_hw_path_pairs);
// both empty: the whole target (isocon_ed_path_pairs).
struct NwpHits {
    std::vector<uint64_t> pair;
    std::vector<uint32_t> q, t;
    std::vector<int32_t> ed, start, cols;
    bool window() const { return !start.empty() || !cols.empty(); }
};

// What both path entries do once the distances (and windows) are known: trace store and slice of reversed runs of every hit, the
// launches of k_nwp_trace cut by the budget, out_ops_ptr, the capacity protocol and k_nwp_emit into out_ops.  extra(p): the ops a
// pair that is no hit owns (the caller writes them after ISOCON_OK).  *kernel_ms gains the time of the launches.
template <class Extra>
int nwp_paths(isocon_store *s, const char *who, const char *lap, const NwpHits &H, uint64_t n_pairs, Extra extra, uint32_t *out_ops, uint64_t *out_ops_ptr,
              uint64_t ops_cap, uint64_t *needed, float *kernel_ms, HostClock &clk)
{
    const std::vector<int32_t> &lens = s->lens;
    const bool window = H.window();
    const std::string name(who), stage(lap);
    const size_t nh = H.pair.size();
    int rc;
    uint64_t budget = kNwpTraceBudget;
    if (const char *e = variant_value("nwp_trace_budget")) budget = strtoull(e, nullptr, 10);
    std::vector<uint64_t> units(nh), rev_off(nh);
    uint64_t rev_total = 0;
    size_t lds = 0;
    for (size_t i = 0; i < nh; ++i) {
        const int32_t m = lens[H.q[i]], nt = lens[H.t[i]], nc = window ? H.cols[i] : nt;
        if (window && (H.start[i] < 0 || nc <= 0 || nc > nt - H.start[i])) {
            g_last_error = name + ": internal status (window) for pair " + std::to_string(H.pair[i]);
            return ISOCON_E_HIP;
        }
        const uint64_t u = hwf_trace_units(m, nc);
        if (u * 16 > budget) {
            g_last_error = name + ": the trace of a query of " + std::to_string(m) + " bases against a target of " + std::to_string(nt) + " bases" +
                           (window ? " (window of " + std::to_string(nc) + " columns)" : std::string()) + " needs " + std::to_string(u * 16) + " bytes (budget " +
                           std::to_string(budget) + ")";
            return ISOCON_E_UNSUPPORTED;
        }
        if (hwf_passes(m) > 1) lds = std::max(lds, (size_t)hwf_bound_words(nc) * 4);
        units[i] = u;
        rev_off[i] = rev_total;
        rev_total += nwp_max_runs(H.ed[i]);
    }
    if (lds > kHwfMaxLds) {
        g_last_error = name + ": a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
        return ISOCON_E_UNSUPPORTED;
    }
    std::vector<int32_t> runs(nh, 0);
    EventTimer tm;
    ScratchPool *pl = &s->pool;
    DevBuf d_q(pl, SLOT_NWP_Q), d_t(pl, SLOT_NWP_T), d_ed(pl, SLOT_NWP_ED), d_toff(pl, SLOT_NWP_TOFF), d_roff(pl, SLOT_NWP_ROFF), d_rev(pl, SLOT_NWP_REV),
        d_runs(pl, SLOT_NWP_RUNS), d_foff(pl, SLOT_NWP_FOFF), d_ops(pl, SLOT_NWP_OPS), d_trace(pl, SLOT_HW_TRACE), d_start(pl, SLOT_NWP_START),
        d_cols(pl, SLOT_NWP_COLS);
    size_t launches = 0;
    uint64_t trace_bytes = 0;
    if (nh) {
        // the launches: consecutive hits whose stores fit the budget together; trace_off is relative to its launch
        std::vector<uint64_t> toff(nh);
        std::vector<size_t> cut(1, 0);
        uint64_t total = 0, most = 0;
        for (size_t i = 0; i < nh; ++i) {
            if ((total + units[i]) * 16 > budget || i - cut.back() >= ((size_t)1 << 20)) { cut.push_back(i); total = 0; }
            toff[i] = total; total += units[i];
            most = std::max(most, total);
            trace_bytes += units[i] * 16;
        }
        cut.push_back(nh);
        if ((rc = d_q.alloc(nh * 4)) || (rc = d_t.alloc(nh * 4)) || (rc = d_ed.alloc(nh * 4)) || (rc = d_toff.alloc(nh * 8)) || (rc = d_roff.alloc(nh * 8)) ||
            (rc = d_rev.alloc((size_t)rev_total * 4)) || (rc = d_runs.alloc(nh * 4)) || (rc = d_trace.alloc((size_t)most * 16)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_q.p, H.q.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_t.p, H.t.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_ed.p, H.ed.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_toff.p, toff.data(), nh * 8));
        ISO_HIP_CHECK(copy_h2d(d_roff.p, rev_off.data(), nh * 8));
        if (window) {
            if ((rc = d_start.alloc(nh * 4)) || (rc = d_cols.alloc(nh * 4))) return rc;
            ISO_HIP_CHECK(copy_h2d(d_start.p, H.start.data(), nh * 4));
            ISO_HIP_CHECK(copy_h2d(d_cols.p, H.cols.data(), nh * 4));
        }
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
        ISO_HIP_CHECK(copy_d2h(runs.data(), d_runs.p, nh * 4));
        for (size_t i = 0; i < nh; ++i)
            if (runs[i] <= 0 || (uint64_t)runs[i] > nwp_max_runs(H.ed[i])) {
                g_last_error = name + ": internal status " + std::to_string(runs[i]) + " for pair " + std::to_string(H.pair[i]);
                return ISOCON_E_HIP;
            }
    }
    if (clk.on) fprintf(stderr, "[isocon] %s: %llu pairs, %zu traced, %zu launches, %llu bytes of trace\n", lap, (unsigned long long)n_pairs, nh, launches, (unsigned long long)trace_bytes);
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
        if (kernel_ms) *kernel_ms += tm.total;
        g_last_error = name + ": " + std::to_string(total_ops) + " ops, room for " + std::to_string(ops_cap);
        return ISOCON_E_CAPACITY;
    }
    if (nh) {
        std::vector<uint64_t> foff(nh);
        for (size_t i = 0; i < nh; ++i) foff[i] = out_ops_ptr[H.pair[i]];
        if ((rc = d_foff.alloc(nh * 8)) || (rc = d_ops.alloc((size_t)total_ops * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_foff.p, foff.data(), nh * 8));
        tm.start();
        hipLaunchKernelGGL(k_nwp_emit, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, 0, d_rev.as<uint32_t>(), d_roff.as<uint64_t>(), d_runs.as<int32_t>(),
                           d_foff.as<uint64_t>(), (uint32_t)nh, d_ops.as<uint32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(copy_d2h(out_ops, d_ops.p, (size_t)total_ops * 4));
    }
    if (kernel_ms) *kernel_ms += tm.total;
    clk.lap((stage + ": forward ops").c_str());
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_ed_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                                    int32_t *out_ed, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms)
{
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
