// end_inv_host.inc -- host side of isocon_end_invariant_graph (included by isocon_hip.hip): the invariance graph of the end-invariant
// collapse from the store alone.  Windows, the (pair, shift) survivors of the screen, the pairs' keys and the rows stay in device memory
// (end_inv.hpp); down come n + 1 row offsets, two counters and the edges.

extern "C" int isocon_end_invariant_graph(isocon_store *s, int32_t thr, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t edges_cap, uint64_t *n_edges_needed,
                                          uint64_t *out_counters, float *kernel_ms)
{
    if (!s || !out_row_ptr || (edges_cap && !out_cols)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_edges_needed) *n_edges_needed = 0;
    if (out_counters) for (int c = 0; c < EINV_OUT_COUNTERS; ++c) out_counters[c] = 0;
    if (thr < 0) { g_last_error = "isocon_end_invariant_graph: thr must be >= 0"; return ISOCON_E_ARG; }
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    for (uint32_t i = 1; i < n; ++i)
        if (s->lens[i] < s->lens[i - 1]) { g_last_error = "isocon_end_invariant_graph: the store must be in ascending length order"; return ISOCON_E_ARG; }
    if (thr > EINV_MAX_THR) {
        g_last_error = "isocon_end_invariant_graph: thr " + std::to_string(thr) + " not supported (limit " + std::to_string(EINV_MAX_THR) + ")";
        return ISOCON_E_UNSUPPORTED;
    }
    if (n && s->lens[0] <= thr) {
        g_last_error = "isocon_end_invariant_graph: a sequence of " + std::to_string(s->lens[0]) + " symbols is not longer than thr " + std::to_string(thr);
        return ISOCON_E_UNSUPPORTED;
    }
    for (uint32_t i = 0; i <= n; ++i) out_row_ptr[i] = 0;
    if (n < 2) return ISOCON_OK;
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_lo(pl, SLOT_EINV_LO), d_tot(pl, SLOT_EINV_TOT), d_first(pl, SLOT_EINV_FIRST), d_ctr(pl, SLOT_EINV_CTR);
    int rc;
    if ((rc = d_lo.alloc((size_t)n * 4)) || (rc = d_tot.alloc((size_t)n * 4)) || (rc = d_first.alloc(((size_t)n + 1) * 8)) || (rc = d_ctr.alloc(EINV_DEV_COUNTERS * 8))) return rc;
    EventTimer tm;
    // ---- windows: partners per entry, their scan ----
    tm.start();
    hipLaunchKernelGGL(k_einv_window, dim3((n + 255) / 256), dim3(256), 0, 0, s->d_lens, n, thr, d_lo.as<uint32_t>(), d_tot.as<uint32_t>());
    if ((rc = device_exscan<0, unsigned long long>(pl, d_tot.as<uint32_t>(), n, d_first.as<unsigned long long>()))) return rc;
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    unsigned long long n_pairs = 0;
    ISO_HIP_CHECK(memcpy_wait(&n_pairs, d_first.as<unsigned long long>() + n, 8, hipMemcpyDeviceToHost));
    if (n_pairs > 0xfffffff0ull) { g_last_error = "isocon_end_invariant_graph: more than 0xfffffff0 window pairs"; return ISOCON_E_UNSUPPORTED; }
    uint64_t ctr[EINV_OUT_COUNTERS] = {0};
    ctr[EINV_OUT_PAIRS] = n_pairs;
    if (out_counters) out_counters[EINV_OUT_PAIRS] = n_pairs;
    if (!n_pairs) { if (kernel_ms) *kernel_ms = tm.total; return ISOCON_OK; }
    DevBuf d_best(pl, SLOT_EINV_BEST), d_surv(pl, SLOT_EINV_SURV), d_cnt(pl, SLOT_EINV_ROWCNT), d_rptr(pl, SLOT_EINV_ROWPTR);
    // room for one survivor per pair to begin with: related candidates survive at one shift, unrelated ones at none; a periodic set that
    // survives at many is screened a second time with the room the first run counted
    unsigned long long surv_cap = n_pairs + 1024ull, dctr[EINV_DEV_COUNTERS] = {0, 0};
    if ((rc = d_best.alloc(n_pairs * 4)) || (rc = d_surv.alloc(surv_cap * 8)) || (rc = d_cnt.alloc((size_t)n * 4)) || (rc = d_rptr.alloc(((size_t)n + 1) * 8))) return rc;
    const unsigned pb = (unsigned)((n_pairs + 255) / 256);
    // ---- screen: every shift of every pair on the first 64 bases of its overlap ----
    for (int run = 0; run < 2; ++run) {
        tm.start();
        ISO_HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, EINV_DEV_COUNTERS * 8, 0));
        hipLaunchKernelGGL(k_einv_screen, dim3(pb), dim3(256), 0, 0, s->dev, d_first.as<unsigned long long>(), d_lo.as<uint32_t>(), n_pairs, thr, d_surv.as<uint2>(), surv_cap,
                           d_ctr.as<unsigned long long>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(memcpy_wait(dctr, d_ctr.p, sizeof(dctr), hipMemcpyDeviceToHost));
        if (dctr[EINV_SURVIVORS] <= surv_cap) break;
        if (run == 1 || dctr[EINV_SURVIVORS] > 0xfffffff0ull) {
            g_last_error = "isocon_end_invariant_graph: " + std::to_string(dctr[EINV_SURVIVORS]) + " (pair, shift) candidates after the first-word test";
            return ISOCON_E_UNSUPPORTED;
        }
        surv_cap = dctr[EINV_SURVIVORS];
        if ((rc = d_surv.alloc(surv_cap * 8))) return rc;
    }
    const unsigned long long n_surv = dctr[EINV_SURVIVORS];
    ctr[EINV_OUT_SURVIVORS] = n_surv;
    ctr[EINV_OUT_VERIFIED] = dctr[EINV_VERIFIED];
    clk.lap("einv: screen");
    // ---- verify the survivors, then the rows: count, scan, write ----
    tm.start();
    ISO_HIP_CHECK(hipMemsetAsync(d_best.p, 0xff, n_pairs * 4, 0));
    if (n_surv)
        hipLaunchKernelGGL(k_einv_verify, dim3((unsigned)((n_surv + 255) / 256)), dim3(256), 0, 0, s->dev, d_first.as<unsigned long long>(), d_lo.as<uint32_t>(), d_surv.as<uint2>(),
                           n_surv, d_best.as<uint32_t>());
    hipLaunchKernelGGL((k_einv_rows<false>), dim3((n + 3) / 4), dim3(256), 0, 0, s->d_lens, d_first.as<unsigned long long>(), d_lo.as<uint32_t>(), n, thr, d_best.as<uint32_t>(),
                       d_cnt.as<uint32_t>(), (const unsigned long long *)nullptr, (uint32_t *)nullptr);
    if ((rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), n, d_rptr.as<unsigned long long>()))) return rc;
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "row offsets are copied as they are");
    ISO_HIP_CHECK(memcpy_wait(out_row_ptr, d_rptr.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t n_edges = out_row_ptr[n];
    ctr[EINV_OUT_INVARIANT] = n_edges;
    if (out_counters) for (int c = 0; c < EINV_OUT_COUNTERS; ++c) out_counters[c] = ctr[c];
    if (clk.on) fprintf(stderr, "[isocon] einv: %llu window pairs, %llu (pair, shift) survivors, %llu pairs verified, %llu invariant\n", (unsigned long long)ctr[0],
                        (unsigned long long)ctr[1], (unsigned long long)ctr[2], (unsigned long long)ctr[3]);
    if (n_edges_needed) *n_edges_needed = n_edges;
    if (kernel_ms) *kernel_ms = tm.total;
    if (n_edges > edges_cap) {
        g_last_error = "isocon_end_invariant_graph: " + std::to_string(n_edges) + " edges, room for " + std::to_string(edges_cap);
        return ISOCON_E_CAPACITY;
    }
    if (!n_edges) return ISOCON_OK;
    DevBuf d_cols(pl, SLOT_EINV_COLS);
    if ((rc = d_cols.alloc(n_edges * 4))) return rc;
    tm.start();
    hipLaunchKernelGGL((k_einv_rows<true>), dim3((n + 3) / 4), dim3(256), 0, 0, s->d_lens, d_first.as<unsigned long long>(), d_lo.as<uint32_t>(), n, thr, d_best.as<uint32_t>(),
                       (uint32_t *)nullptr, d_rptr.as<unsigned long long>(), d_cols.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    ISO_HIP_CHECK(copy_d2h(out_cols, d_cols.p, n_edges * 4));
    clk.lap("einv: rows");
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}
