// hw_full_host.inc -- host side of isocon_hw_pairs_wide (included by isocon_hip.hip after hw_host.inc): the pairs whose own band
// fits the 512 diagonals of hw.hpp go through isocon_hw_pairs as one sub-list, the others through the un-banded kernels of hw_full.hpp.

namespace {

// does isocon_hw_pairs take the pair (it needs no kernel, or its band fits)?
inline bool hwf_is_narrow(int32_t len_q, int32_t len_t, int32_t kk)
{
    const int32_t delta = len_t - len_q;
    if (delta < -kk || len_q == 0 || len_t == 0) return true;
    return hwt_words(hw_locate_rows(delta, kk)) != 0;
}

int hwf_pairs(isocon_store *s, const std::vector<uint32_t> &q, const std::vector<uint32_t> &t, const std::vector<int32_t> &k, int32_t *rows, float *kernel_ms)
{
    const size_t nw = q.size();
    const std::vector<int32_t> &lens = s->lens;
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_he(pl, SLOT_HW_Q), d_out(pl, SLOT_HW_OUT), d_trace(pl, SLOT_HW_TRACE);
    DevBuf d_list(pl, SLOT_HW_LANES), d_off(pl, SLOT_HW_TBASE);
    int rc;
    if ((rc = d_q.alloc(nw * 4)) || (rc = d_t.alloc(nw * 4)) || (rc = d_k.alloc(nw * 4)) || (rc = d_he.alloc(nw * 8)) || (rc = d_out.alloc(nw * 20))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_q.p, q.data(), nw * 4));
    ISO_HIP_CHECK(copy_h2d(d_t.p, t.data(), nw * 4));
    ISO_HIP_CHECK(copy_h2d(d_k.p, k.data(), nw * 4));
    // the boundary row between two passes of 64 blocks: 2 bits per column in LDS, only when some query has more than 4 096 rows
    size_t lds = 0;
    for (size_t x = 0; x < nw; ++x)
        if (hwf_passes(lens[q[x]]) > 1) lds = std::max(lds, (size_t)hwf_bound_words(lens[t[x]]) * 4);
    if (lds > kHwfMaxLds) {
        g_last_error = "isocon_hw_pairs_wide: a query of more than 4096 bases against a target of more than " + std::to_string(kHwfMaxLds * 4) + " bases is not supported";
        return ISOCON_E_UNSUPPORTED;
    }
    if (lds > ((size_t)64 << 10)) {
        ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_hwf_locate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_hwf_finish, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    HwfIn in{};
    in.pq = d_q.as<uint32_t>(); in.pt = d_t.as<uint32_t>(); in.pk = d_k.as<int32_t>(); in.n = (uint32_t)nw;
    EventTimer tm;
    // ---- LOCATE ----
    tm.start();
    hipLaunchKernelGGL(k_hwf_locate, dim3((unsigned)std::min<size_t>(nw, (size_t)1 << 20)), dim3(64), lds, 0, s->dev, in, d_he.as<int32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    clk.lap("hw wide: locate");
    std::vector<int32_t> he(nw * 2);
    ISO_HIP_CHECK(copy_d2h(he.data(), d_he.p, nw * 8));
    // ---- START + TRACE + walk for the hits, in launches whose trace stores fit the budget (kHwfTraceBudget and the cut: nwp_plan.hpp; a
    //      pair whose own store exceeds it is refused).  ISOCON_DEBUG_VARIANT=hw_trace_budget=<bytes> (tests: many launches at small shapes) ----
    uint64_t budget = kHwfTraceBudget;
    if (const char *e = variant_value("hw_trace_budget")) budget = strtoull(e, nullptr, 10);
    std::vector<uint32_t> hits;
    std::vector<uint64_t> units;
    for (size_t x = 0; x < nw; ++x) {
        if (he[x * 2] < 0) continue;
        const int32_t m = lens[q[x]], end = he[x * 2 + 1];
        if (end < 0 || end >= lens[t[x]]) { g_last_error = "isocon_hw_pairs_wide: internal status (locate) for wide pair " + std::to_string(x); return ISOCON_E_HIP; }
        const uint64_t u = hwf_trace_units(m, end + 1);
        if (u * 16 > budget) {
            g_last_error = "isocon_hw_pairs_wide: the trace of a query of " + std::to_string(m) + " bases ending at column " + std::to_string(end + 1) + " of a target of " +
                           std::to_string(lens[t[x]]) + " bases needs " + std::to_string(u * 16) + " bytes (budget " + std::to_string(budget) + ")";
            return ISOCON_E_UNSUPPORTED;
        }
        hits.push_back((uint32_t)x);
        units.push_back(u);
    }
    // (the list and the offsets go up once, the store is that of the largest launch, as in nwp_paths)
    const BudgetCut cut = budget_cut(units.data(), units.size(), budget);
    if (!hits.empty()) {
        if ((rc = d_list.alloc(hits.size() * 4)) || (rc = d_off.alloc(hits.size() * 8)) || (rc = d_trace.alloc((size_t)cut.most * 16))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_list.p, hits.data(), hits.size() * 4));
        ISO_HIP_CHECK(copy_h2d(d_off.p, cut.off.data(), hits.size() * 8));
    }
    for (size_t c = 0; c + 1 < cut.cut.size(); ++c) {
        const size_t a = cut.cut[c], cnt = cut.cut[c + 1] - a;
        in.list = d_list.as<uint32_t>() + a; in.trace_off = d_off.as<uint64_t>() + a; in.n = (uint32_t)cnt;
        tm.start();
        hipLaunchKernelGGL(k_hwf_finish, dim3((unsigned)cnt), dim3(64), lds, 0, s->dev, in, d_he.as<int32_t>(), d_trace.as<ulonglong2>(), d_out.as<int32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();                                      // also the fence before the next launch reuses the store
    }
    if (clk.on) fprintf(stderr, "[isocon] hw wide: %zu pairs, %zu hits, %zu finish launches\n", nw, hits.size(), cut.launches());
    clk.lap("hw wide: finish");
    std::vector<int32_t> res;
    if (!hits.empty()) {
        res.resize(nw * 5);
        ISO_HIP_CHECK(copy_d2h(res.data(), d_out.p, nw * 20));
    }
    for (size_t x = 0; x < nw; ++x) {
        int32_t *o = rows + x * 5;
        o[0] = -1; o[1] = -1; o[2] = -1; o[3] = 0; o[4] = 0;
    }
    for (uint32_t x : hits) {
        const int32_t *r = res.data() + (size_t)x * 5;
        if (r[0] < -1) { g_last_error = "isocon_hw_pairs_wide: internal status " + std::to_string(r[0]) + " for wide pair " + std::to_string(x); return ISOCON_E_HIP; }
        for (int i = 0; i < 5; ++i) rows[(size_t)x * 5 + i] = r[i];
    }
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_hw_pairs_wide(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                                    int32_t *out, float *kernel_ms)
{
    if (!s || (n_pairs && (!q || !t || !k || !out))) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!n_pairs) return ISOCON_OK;
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    if (n_pairs > 0xfffffff0ull) return ISOCON_E_UNSUPPORTED;
    const uint32_t n = s->dev.n;
    const std::vector<int32_t> &lens = s->lens;
    std::vector<uint64_t> wide;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (q[p] >= n || t[p] >= n) return ISOCON_E_ARG;
        if (k[p] < 0) { g_last_error = "isocon_hw_pairs_wide: k must be >= 0"; return ISOCON_E_ARG; }
        if (k[p] > (1 << 20)) return ISOCON_E_UNSUPPORTED;
        if (!hwf_is_narrow(lens[q[p]], lens[t[p]], k[p])) wide.push_back(p);
    }
    if (wide.empty()) return isocon_hw_pairs(s, q, t, k, n_pairs, out, kernel_ms);
    float ms_narrow = 0.f, ms_wide = 0.f;
    int rc;
    // the narrow pairs, in their order, as one call of the banded implementation
    const uint64_t n_narrow = n_pairs - wide.size();
    if (n_narrow) {
        std::vector<uint32_t> nq(n_narrow), nt(n_narrow);
        std::vector<int32_t> nk(n_narrow), rows(n_narrow * 5);
        std::vector<uint64_t> at(n_narrow);
        size_t w = 0, c = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            if (w < wide.size() && wide[w] == p) { ++w; continue; }
            nq[c] = q[p]; nt[c] = t[p]; nk[c] = k[p]; at[c] = p; ++c;
        }
        if ((rc = isocon_hw_pairs(s, nq.data(), nt.data(), nk.data(), n_narrow, rows.data(), &ms_narrow))) return rc;
        for (size_t i = 0; i < n_narrow; ++i) memcpy(out + at[i] * 5, rows.data() + i * 5, 20);
    }
    {
        const size_t nw = wide.size();
        std::vector<uint32_t> wq(nw), wt(nw);
        std::vector<int32_t> wk(nw), rows(nw * 5);
        for (size_t i = 0; i < nw; ++i) { wq[i] = q[wide[i]]; wt[i] = t[wide[i]]; wk[i] = k[wide[i]]; }
        if ((rc = hwf_pairs(s, wq, wt, wk, rows.data(), &ms_wide))) return rc;
        for (size_t i = 0; i < nw; ++i) memcpy(out + wide[i] * 5, rows.data() + i * 5, 20);
    }
    if (kernel_ms) *kernel_ms = ms_narrow + ms_wide;
    return ISOCON_OK;
}
