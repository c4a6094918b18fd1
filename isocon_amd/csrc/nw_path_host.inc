// nw_path_host.inc -- host side of isocon_ed_path_pairs (included by isocon_hip.hip after hw_full_host.inc): the bounded distances
// through the implementation of isocon_ed_pairs, then the paths of the pairs within their threshold through nw_path.hpp.

namespace {

// Trace scratch one launch of k_nwp_trace may hold (SLOT_HW_TRACE, shared with the un-banded infix kernels): the host cuts the hits
// into as many launches as that takes, a pair whose own store exceeds it is refused.  ISOCON_DEBUG_VARIANT=nwp_trace_budget=<bytes>
// (tests: many launches at small shapes).  The LDS limit of the boundary row is kHwfMaxLds.
static constexpr uint64_t kNwpTraceBudget = (uint64_t)1 << 30;

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
    // ---- the hits: trace store and slice of reversed runs of each ----
    uint64_t budget = kNwpTraceBudget;
    if (const char *e = variant_value("nwp_trace_budget")) budget = strtoull(e, nullptr, 10);
    std::vector<uint64_t> hits;
    std::vector<uint32_t> hq, ht;
    std::vector<int32_t> hed;
    std::vector<uint64_t> units, rev_off;
    uint64_t rev_total = 0;
    size_t lds = 0;
    for (uint64_t p : full) {
        if (out_ed[p] < 0) continue;
        const int32_t m = lens[q[p]], nt = lens[t[p]];
        const uint64_t u = hwf_trace_units(m, nt);
        if (u * 16 > budget) {
            g_last_error = "isocon_ed_path_pairs: the trace of a query of " + std::to_string(m) + " bases against a target of " + std::to_string(nt) + " bases needs " +
                           std::to_string(u * 16) + " bytes (budget " + std::to_string(budget) + ")";
            return ISOCON_E_UNSUPPORTED;
        }
        if (hwf_passes(m) > 1) lds = std::max(lds, (size_t)hwf_bound_words(nt) * 4);
        hits.push_back(p); hq.push_back(q[p]); ht.push_back(t[p]); hed.push_back(out_ed[p]);
        units.push_back(u);
        rev_off.push_back(rev_total);
        rev_total += nwp_max_runs(out_ed[p]);
    }
    if (lds > kHwfMaxLds) {
        g_last_error = "isocon_ed_path_pairs: a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
        return ISOCON_E_UNSUPPORTED;
    }
    const size_t nh = hits.size();
    std::vector<int32_t> runs(nh, 0);
    EventTimer tm;
    ScratchPool *pl = &s->pool;
    DevBuf d_q(pl, SLOT_NWP_Q), d_t(pl, SLOT_NWP_T), d_ed(pl, SLOT_NWP_ED), d_toff(pl, SLOT_NWP_TOFF), d_roff(pl, SLOT_NWP_ROFF), d_rev(pl, SLOT_NWP_REV),
        d_runs(pl, SLOT_NWP_RUNS), d_foff(pl, SLOT_NWP_FOFF), d_ops(pl, SLOT_NWP_OPS), d_trace(pl, SLOT_HW_TRACE);
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
        ISO_HIP_CHECK(copy_h2d(d_q.p, hq.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_t.p, ht.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_ed.p, hed.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_toff.p, toff.data(), nh * 8));
        ISO_HIP_CHECK(copy_h2d(d_roff.p, rev_off.data(), nh * 8));
        if (lds > ((size_t)64 << 10)) ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nwp_trace, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            const size_t a = cut[c], cnt = cut[c + 1] - a;
            NwpIn in{};
            in.pq = d_q.as<uint32_t>() + a; in.pt = d_t.as<uint32_t>() + a; in.ed = d_ed.as<int32_t>() + a;
            in.trace_off = d_toff.as<uint64_t>() + a; in.rev_off = d_roff.as<uint64_t>() + a; in.n = (uint32_t)cnt;
            tm.start();
            hipLaunchKernelGGL(k_nwp_trace, dim3((unsigned)cnt), dim3(64), lds, 0, s->dev, in, d_trace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>() + a);
            ISO_HIP_CHECK(hipGetLastError());
            tm.stop();                                      // also the fence before the next launch reuses the store
            ++launches;
        }
        ISO_HIP_CHECK(copy_d2h(runs.data(), d_runs.p, nh * 4));
        for (size_t i = 0; i < nh; ++i)
            if (runs[i] <= 0 || (uint64_t)runs[i] > nwp_max_runs(hed[i])) {
                g_last_error = "isocon_ed_path_pairs: internal status " + std::to_string(runs[i]) + " for pair " + std::to_string(hits[i]);
                return ISOCON_E_HIP;
            }
    }
    if (clk.on) fprintf(stderr, "[isocon] ed path: %llu pairs, %zu traced, %zu launches, %llu bytes of trace\n", (unsigned long long)n_pairs, nh, launches, (unsigned long long)trace_bytes);
    clk.lap("ed path: trace + walk");
    // ---- offsets of the dense forward list: a traced pair has its runs, a hit with an empty sequence one op (none if both are) ----
    {
        size_t h = 0;
        uint64_t at = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            out_ops_ptr[p] = at;
            if (h < nh && hits[h] == p) at += (uint64_t)runs[h++];
            else if (out_ed[p] > 0 && (lens[q[p]] == 0 || lens[t[p]] == 0)) at += 1;
        }
        out_ops_ptr[n_pairs] = at;
    }
    const uint64_t total_ops = out_ops_ptr[n_pairs];
    if (needed) *needed = total_ops;
    if (kernel_ms) *kernel_ms = ms_ed + tm.total;
    if (total_ops > ops_cap) {
        g_last_error = "isocon_ed_path_pairs: " + std::to_string(total_ops) + " ops, room for " + std::to_string(ops_cap);
        return ISOCON_E_CAPACITY;
    }
    if (nh) {
        std::vector<uint64_t> foff(nh);
        for (size_t i = 0; i < nh; ++i) foff[i] = out_ops_ptr[hits[i]];
        if ((rc = d_foff.alloc(nh * 8)) || (rc = d_ops.alloc((size_t)total_ops * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_foff.p, foff.data(), nh * 8));
        tm.start();
        hipLaunchKernelGGL(k_nwp_emit, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, 0, d_rev.as<uint32_t>(), d_roff.as<uint64_t>(), d_runs.as<int32_t>(),
                           d_foff.as<uint64_t>(), (uint32_t)nh, d_ops.as<uint32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(copy_d2h(out_ops, d_ops.p, (size_t)total_ops * 4));
    }
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const int32_t m = lens[q[p]], nt = lens[t[p]];
        if (out_ed[p] > 0 && (m == 0 || nt == 0)) out_ops[out_ops_ptr[p]] = m == 0 ? nwp_op(NWP_D, nt) : nwp_op(NWP_I, m);
    }
    if (kernel_ms) *kernel_ms = ms_ed + tm.total;
    clk.lap("ed path: forward ops");
    return ISOCON_OK;
}
