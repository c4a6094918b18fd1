// nw_path_host.inc -- host side of isocon_ed_path_pairs (included by isocon_hip.hip after hw_full_host.inc): the bounded distances
// through the implementation of isocon_ed_pairs, then the paths of the pairs within their threshold through nw_band.hpp (the hits whose
// corridor fits 256 diagonals) and nw_path.hpp (the others).  nwp_paths, the driver of that second part, is shared with
// isocon_hw_path_pairs (hw_path_host.inc) and isocon_shw_path_pairs (shw_host.inc), whose hits are traced over a window; what it decides
// without a device (classes, budgets, order, waves, launches, offsets) is in nwp_plan.hpp.

namespace {

// isocon_path_last_stats: the calling thread's last path call.
enum { PS_HITS = 0, PS_W1, PS_W2, PS_W4, PS_UNBANDED, PS_BYTES_BAND, PS_BYTES_UNBANDED, PS_LAUNCHES_BAND, PS_LAUNCHES_UNBANDED, PS_MS_BAND, PS_MS_UNBANDED, PS_MS_EMIT,
       PS_COUNT };
thread_local double g_path_stats[PS_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
// A call that traces nothing, or fails before or while its hits are classed, reports zeros.
inline void path_stats_reset() { for (double &x : g_path_stats) x = 0; }

// What the three path entries do first: the stats reset, the pointer test (per_pair: the arrays the entry needs of a list that is not
// empty), zeros in *kernel_ms, *needed and out_ops_ptr[0], the empty list.  true: the call is over, with *status.
inline bool path_prologue(const void *s, uint64_t n_pairs, std::initializer_list<const void *> per_pair, const uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap,
                          uint64_t *needed, float *kernel_ms, int *status)
{
    path_stats_reset();
    bool ok = s && out_ops_ptr && (!ops_cap || out_ops);
    for (const void *a : per_pair) ok = ok && (!n_pairs || a);
    *status = ok ? ISOCON_OK : ISOCON_E_ARG;
    if (!ok) return true;
    if (kernel_ms) *kernel_ms = 0.f;
    if (needed) *needed = 0;
    out_ops_ptr[0] = 0;
    return n_pairs == 0;
}

template <int W>
void nwb_launch(bool window, unsigned waves, const DevStore &dev, const NwbIn &in, ulonglong2 *trace, uint32_t *rev, int32_t *runs)
{
    if (window) hipLaunchKernelGGL((k_nwb_trace<W, true>), dim3(waves), dim3(64), 0, 0, dev, in, trace, rev, runs);
    else hipLaunchKernelGGL((k_nwb_trace<W, false>), dim3(waves), dim3(64), 0, 0, dev, in, trace, rev, runs);
}

// What the path entries do once the distances (and windows) are known: the plan of nwp_plan.hpp, then its launches of k_nwp_trace and
// k_nwb_trace, out_ops_ptr, the capacity protocol and k_nwp_emit into out_ops.
// extra(p): the ops a pair that is no hit owns (the caller writes them after ISOCON_OK).  *kernel_ms gains the time of the launches.
template <class Extra>
int nwp_paths(isocon_store *s, const char *who, const char *lap, const NwpHits &H, uint64_t n_pairs, Extra extra, uint32_t *out_ops, uint64_t *out_ops_ptr,
              uint64_t ops_cap, uint64_t *needed, float *kernel_ms, HostClock &clk)
{
    const bool window = H.window();
    const std::string name(who), stage(lap);
    const size_t nh = H.pair.size();
    int rc;
    path_stats_reset();
    // ISOCON_DEBUG_VARIANT=nwp_trace_budget=<bytes> / nwp_band_budget=<bytes> (tests: many launches at small shapes).  nwp_unbanded sends
    // every hit through k_nwp_trace; nwp_trace_budget= implies it (whoever sets that budget means that store).
    uint64_t budget = kNwpTraceBudget, band_budget = kNwpBandBudget;
    bool unbanded = variant("nwp_unbanded");
    if (const char *e = variant_value("nwp_trace_budget")) { budget = strtoull(e, nullptr, 10); unbanded = true; }
    if (const char *e = variant_value("nwp_band_budget")) band_budget = strtoull(e, nullptr, 10);
    NwpPlan P;
    std::string refusal;
    if ((rc = nwp_plan(s->lens, H, budget, band_budget, unbanded, P, refusal))) { g_last_error = name + ": " + refusal; return rc; }
    const size_t nu = P.nu, nw = P.wcols.size(), lds = P.lds;
    g_path_stats[PS_HITS] = (double)nh; g_path_stats[PS_UNBANDED] = (double)nu;
    g_path_stats[PS_W1] = P.per_class[1]; g_path_stats[PS_W2] = P.per_class[2]; g_path_stats[PS_W4] = P.per_class[4];
    EventTimer tm, tm_band, tm_emit;
    ScratchPool *pl = &s->pool;
    DevBuf d_q(pl, SLOT_NWP_Q), d_t(pl, SLOT_NWP_T), d_ed(pl, SLOT_NWP_ED), d_toff(pl, SLOT_NWP_TOFF), d_roff(pl, SLOT_NWP_ROFF), d_rev(pl, SLOT_NWP_REV),
        d_runs(pl, SLOT_NWP_RUNS), d_foff(pl, SLOT_NWP_FOFF), d_ops(pl, SLOT_NWP_OPS), d_trace(pl, SLOT_HW_TRACE), d_start(pl, SLOT_NWP_START),
        d_cols(pl, SLOT_NWP_COLS), d_btrace(pl, SLOT_NWB_TRACE), d_slots(pl, SLOT_NWB_SLOTS), d_woff(pl, SLOT_NWB_WOFF), d_wcols(pl, SLOT_NWB_WCOLS),
        d_wlanes(pl, SLOT_NWB_WLANES);
    if (nh) {
        if ((rc = d_q.alloc(nh * 4)) || (rc = d_t.alloc(nh * 4)) || (rc = d_ed.alloc(nh * 4)) || (rc = d_roff.alloc(nh * 8)) ||
            (rc = d_rev.alloc((size_t)P.rev_total * 4)) || (rc = d_runs.alloc(nh * 4)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_q.p, P.pq.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_t.p, P.pt.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_ed.p, P.ped.data(), nh * 4));
        ISO_HIP_CHECK(copy_h2d(d_roff.p, P.rev_off.data(), nh * 8));
        if (window) {
            if ((rc = d_start.alloc(nh * 4)) || (rc = d_cols.alloc(nh * 4))) return rc;
            ISO_HIP_CHECK(copy_h2d(d_start.p, P.pstart.data(), nh * 4));
            ISO_HIP_CHECK(copy_h2d(d_cols.p, P.pcols.data(), nh * 4));
        }
    }
    if (nu) {
        // the un-banded launches (positions 0 .. nu - 1); trace_off is relative to its launch
        const BudgetCut &U = P.unbanded;
        if ((rc = d_toff.alloc(nu * 8)) || (rc = d_trace.alloc((size_t)U.most * 16))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_toff.p, U.off.data(), nu * 8));
        const void *kern = window ? (const void *)k_nwp_trace<true> : (const void *)k_nwp_trace<false>;
        if (lds > ((size_t)64 << 10)) ISO_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        for (size_t c = 0; c + 1 < U.cut.size(); ++c) {
            const size_t a = U.cut[c], cnt = U.cut[c + 1] - a;
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
        }
    }
    if (nw) {
        // the band launches (positions nu .. nh - 1): waves of one class each
        const BudgetCut &B = P.band;
        if ((rc = d_slots.alloc(nw * 64 * 4)) || (rc = d_woff.alloc(nw * 8)) || (rc = d_wcols.alloc(nw * 4)) || (rc = d_wlanes.alloc(nw * 4)) ||
            (rc = d_btrace.alloc((size_t)B.most * 16)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_slots.p, P.slots.data(), nw * 64 * 4));
        ISO_HIP_CHECK(copy_h2d(d_woff.p, B.off.data(), nw * 8));
        ISO_HIP_CHECK(copy_h2d(d_wcols.p, P.wcols.data(), nw * 4));
        ISO_HIP_CHECK(copy_h2d(d_wlanes.p, P.wlanes.data(), nw * 4));
        for (size_t c = 0; c + 1 < B.cut.size(); ++c) {
            const size_t a = B.cut[c], cnt = B.cut[c + 1] - a;
            NwbIn in{};
            in.slot_hit = d_slots.as<uint32_t>() + a * 64; in.wave_off = d_woff.as<uint64_t>() + a; in.wave_cols = d_wcols.as<int32_t>() + a;
            in.wave_lanes = d_wlanes.as<int32_t>() + a;
            in.pq = d_q.as<uint32_t>(); in.pt = d_t.as<uint32_t>(); in.ed = d_ed.as<int32_t>(); in.rev_off = d_roff.as<uint64_t>();
            in.t_start = window ? d_start.as<int32_t>() : nullptr; in.t_cols = window ? d_cols.as<int32_t>() : nullptr;
            in.n_waves = (uint32_t)cnt;
            tm_band.start();
            const int32_t W = P.wcls[a];
            if (W == 1) nwb_launch<1>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            else if (W == 2) nwb_launch<2>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            else nwb_launch<4>(window, (unsigned)cnt, s->dev, in, d_btrace.as<ulonglong2>(), d_rev.as<uint32_t>(), d_runs.as<int32_t>());
            ISO_HIP_CHECK(hipGetLastError());
            tm_band.stop();                                 // also the fence before the next launch reuses the store
        }
    }
    std::vector<int32_t> runs(nh, 0);          // by hit
    if (nh) {
        std::vector<int32_t> got(nh);          // by position
        ISO_HIP_CHECK(copy_d2h(got.data(), d_runs.p, nh * 4));
        for (size_t p = 0; p < nh; ++p) {
            if (got[p] <= 0 || (uint64_t)got[p] > nwp_max_runs(P.ped[p])) {
                g_last_error = name + ": internal status " + std::to_string(got[p]) + " for pair " + std::to_string(H.pair[P.ord[p]]);
                return ISOCON_E_HIP;
            }
            runs[P.ord[p]] = got[p];
        }
    }
    const size_t launches = P.unbanded.launches(), band_launches = P.band.launches();
    const uint64_t trace_bytes = P.unbanded.sum * 16, band_bytes = P.band.sum * 16;
    g_path_stats[PS_BYTES_BAND] = (double)band_bytes; g_path_stats[PS_BYTES_UNBANDED] = (double)trace_bytes;
    g_path_stats[PS_LAUNCHES_BAND] = (double)band_launches; g_path_stats[PS_LAUNCHES_UNBANDED] = (double)launches;
    g_path_stats[PS_MS_BAND] = tm_band.total; g_path_stats[PS_MS_UNBANDED] = tm.total;
    if (clk.on)
        fprintf(stderr, "[isocon] %s: %llu pairs, %zu traced (%zu un-banded), %zu + %zu launches, %llu + %llu bytes of trace\n", lap, (unsigned long long)n_pairs, nh, nu,
                band_launches, launches, (unsigned long long)band_bytes, (unsigned long long)trace_bytes);
    clk.lap((stage + ": trace + walk").c_str());
    std::vector<uint64_t> foff;          // by position, like the reversed runs
    nwp_forward_offsets(H, P.ord, runs, n_pairs, extra, out_ops_ptr, foff);
    const uint64_t total_ops = out_ops_ptr[n_pairs];
    if (needed) *needed = total_ops;
    if (total_ops > ops_cap) {
        if (kernel_ms) *kernel_ms += tm.total + tm_band.total;
        g_last_error = name + ": " + std::to_string(total_ops) + " ops, room for " + std::to_string(ops_cap);
        return ISOCON_E_CAPACITY;
    }
    if (nh) {
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

extern "C" int isocon_path_last_stats(double *out, int32_t cap) { return copy_last_stats(g_path_stats, PS_COUNT, out, cap); }

extern "C" int isocon_ed_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                                    int32_t *out_ed, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms)
{
    int rc;
    if (path_prologue(s, n_pairs, {q, t, out_ed}, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms, &rc)) return rc;          // (k may be null: unbounded)
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
    if (!full.empty()) {
        const size_t nf = full.size();
        std::vector<uint32_t> fq(nf), ft(nf);
        std::vector<int32_t> fk(nf), fe(nf, -1);
        for (size_t i = 0; i < nf; ++i) { fq[i] = q[full[i]]; ft[i] = t[full[i]]; fk[i] = k ? k[full[i]] : -1; }
        if ((rc = ed_pairs_impl(s, fq.data(), ft.data(), fk.data(), nf, fe.data(), &ms_ed, nullptr, false))) return rc;
        for (size_t i = 0; i < nf; ++i) out_ed[full[i]] = fe[i] < 0 ? -1 : fe[i];
    }
    clk.lap("ed path: distances");
    // ---- the hits, then what the path entries share ----
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
