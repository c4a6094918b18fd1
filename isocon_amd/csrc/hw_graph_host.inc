// hw_graph_host.inc -- host side of isocon_hw_window_graph (included by isocon_hip.hip): the candidate-vs-candidate graph with ignored
// ends from the store alone.  Pairs, rows, end rules and edges stay in device memory (hw_graph.hpp); the rows come from the device
// tile route of isocon_hw_pairs (hw_pairs_device_core, hw_host.inc).  Down come n + 1 row offsets and the edges.

extern "C" int isocon_hw_window_graph(isocon_store *s, int32_t window, int32_t k, uint64_t depth, int32_t end_threshold, int32_t max_ed, int32_t symmetric,
                                      uint64_t *out_row_ptr, uint32_t *out_cols, int32_t *out_ed, uint64_t edges_cap, uint64_t *n_edges_needed,
                                      uint64_t *out_counters, float *kernel_ms)
{
    if (!s || !out_row_ptr || (edges_cap && (!out_cols || !out_ed))) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_edges_needed) *n_edges_needed = 0;
    if (out_counters) for (int c = 0; c < HWG_COUNTERS; ++c) out_counters[c] = 0;
    if (window < 0 || k < 0 || end_threshold < 0 || max_ed < 0) { g_last_error = "isocon_hw_window_graph: window, k, end_threshold and max_ed must be >= 0"; return ISOCON_E_ARG; }
    if (s->n_exc) { g_last_error = "infix alignments run on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    for (uint32_t i = 1; i < n; ++i)
        if (s->lens[i] < s->lens[i - 1]) { g_last_error = "isocon_hw_window_graph: the store must be in ascending length order"; return ISOCON_E_ARG; }
    // the widest band a pair of the window can need (target longer by `window`)
    if ((int64_t)window + 2 * (int64_t)k + 1 > 512) {
        g_last_error = "isocon_hw_window_graph: band of " + std::to_string((int64_t)window + 2 * (int64_t)k + 1) + " diagonals not supported (limit 512)";
        return ISOCON_E_UNSUPPORTED;
    }
    for (uint32_t i = 0; i <= n; ++i) out_row_ptr[i] = 0;
    if (n < 2) return ISOCON_OK;
    HostClock clk;
    ScratchPool *pl = &g_scratch;
    DevBuf d_cd(pl, SLOT_HWG_CD), d_tot(pl, SLOT_HWG_TOT), d_first(pl, SLOT_HWG_FIRST), d_ctr(pl, SLOT_HWG_CTR);
    int rc;
    if ((rc = d_cd.alloc((size_t)n * 4)) || (rc = d_tot.alloc((size_t)n * 4)) || (rc = d_first.alloc(((size_t)n + 1) * 8)) || (rc = d_ctr.alloc(HWG_COUNTERS * 8))) return rc;
    EventTimer tm;
    float ms_rows = 0.f;
    // ---- pairs: counts per entry, their scan, one thread per slot ----
    tm.start();
    ISO_HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, HWG_COUNTERS * 8, 0));
    hipLaunchKernelGGL(k_hwg_counts, dim3((n + 255) / 256), dim3(256), 0, 0, s->d_lens, n, window, hwg_jmax(depth, n), d_cd.as<uint32_t>(), d_tot.as<uint32_t>());
    if ((rc = device_exscan<0, unsigned long long>(pl, d_tot.as<uint32_t>(), n, d_first.as<unsigned long long>()))) return rc;
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    unsigned long long n_pairs = 0;
    ISO_HIP_CHECK(memcpy_wait(&n_pairs, d_first.as<unsigned long long>() + n, 8, hipMemcpyDeviceToHost));
    uint64_t ctr[HWG_COUNTERS] = {0};
    ctr[HWG_PAIRS] = n_pairs;
    if (n_pairs > 0xfffffff0ull) { g_last_error = "isocon_hw_window_graph: more than 0xfffffff0 pairs"; return ISOCON_E_UNSUPPORTED; }
    if (!n_pairs) { if (kernel_ms) *kernel_ms = tm.total; if (out_counters) out_counters[HWG_PAIRS] = 0; return ISOCON_OK; }
    DevBuf d_q(pl, SLOT_HW_PQ), d_t(pl, SLOT_HW_T), d_k(pl, SLOT_HW_K), d_val(pl, SLOT_HWG_VALUE), d_cnt(pl, SLOT_HWG_ROWCNT), d_rptr(pl, SLOT_HWG_ROWPTR);
    if ((rc = d_q.alloc(n_pairs * 4)) || (rc = d_t.alloc(n_pairs * 4)) || (rc = d_k.alloc(n_pairs * 4)) || (rc = d_val.alloc(n_pairs * 4)) ||
        (rc = d_cnt.alloc((size_t)n * 4)) || (rc = d_rptr.alloc(((size_t)n + 1) * 8)))
        return rc;
    const unsigned pb = (unsigned)((n_pairs + 255) / 256);
    tm.start();
    hipLaunchKernelGGL(k_hwg_pairs, dim3(pb), dim3(256), 0, 0, d_first.as<unsigned long long>(), d_cd.as<uint32_t>(), n, n_pairs, k, d_q.as<uint32_t>(), d_t.as<uint32_t>(),
                       d_k.as<int32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    clk.lap("hwg: pairs (device)");
    // ---- rows: the launches of isocon_hw_pairs on the device-resident lists ----
    int32_t *d_rows = nullptr;
    bool retry_host = false;
    rc = hw_pairs_device_core(s, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_k.as<int32_t>(), n_pairs, &d_rows, &ms_rows, &retry_host);
    if (rc) {
        if (retry_host) g_last_error = "isocon_hw_window_graph: the tiles of this list cannot be formed on the device";
        return rc;
    }
    clk.lap("hwg: rows");
    // ---- end rules, then the edges: count, scan, write ----
    tm.start();
    hipLaunchKernelGGL(k_hwg_adjust, dim3(pb), dim3(256), 0, 0, s->d_lens, d_q.as<uint32_t>(), d_t.as<uint32_t>(), d_rows, n_pairs, k, end_threshold, max_ed,
                       d_val.as<int32_t>(), d_ctr.as<unsigned long long>());
    hipLaunchKernelGGL((k_hwg_edges<false>), dim3((n + 3) / 4), dim3(256), 0, 0, d_first.as<unsigned long long>(), d_cd.as<uint32_t>(), n, d_val.as<int32_t>(), symmetric,
                       d_cnt.as<uint32_t>(), (const unsigned long long *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr, d_ctr.as<unsigned long long>());
    if ((rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), n, d_rptr.as<unsigned long long>()))) return rc;
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "row offsets are copied as they are");
    ISO_HIP_CHECK(memcpy_wait(out_row_ptr, d_rptr.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    {
        unsigned long long dctr[HWG_COUNTERS];
        ISO_HIP_CHECK(memcpy_wait(dctr, d_ctr.p, sizeof(dctr), hipMemcpyDeviceToHost));
        for (int c = HWG_NEED_KERNEL; c < HWG_COUNTERS; ++c) ctr[c] = dctr[c];
    }
    if (out_counters) for (int c = 0; c < HWG_COUNTERS; ++c) out_counters[c] = ctr[c];
    const uint64_t n_edges = out_row_ptr[n];
    if (clk.on) fprintf(stderr, "[isocon] hwg: %llu pairs, %llu need a kernel, %llu hits, %llu directed edges, %llu appended\n", (unsigned long long)ctr[0],
                        (unsigned long long)ctr[1], (unsigned long long)ctr[2], (unsigned long long)ctr[3], (unsigned long long)ctr[4]);
    if (n_edges_needed) *n_edges_needed = n_edges;
    if (kernel_ms) *kernel_ms = tm.total + ms_rows;
    if (n_edges > edges_cap) {
        g_last_error = "isocon_hw_window_graph: " + std::to_string(n_edges) + " edges, room for " + std::to_string(edges_cap);
        return ISOCON_E_CAPACITY;
    }
    if (!n_edges) return ISOCON_OK;
    DevBuf d_cols(pl, SLOT_HWG_COLS), d_ed(pl, SLOT_HWG_ED);
    if ((rc = d_cols.alloc(n_edges * 4)) || (rc = d_ed.alloc(n_edges * 4))) return rc;
    tm.start();
    hipLaunchKernelGGL((k_hwg_edges<true>), dim3((n + 3) / 4), dim3(256), 0, 0, d_first.as<unsigned long long>(), d_cd.as<uint32_t>(), n, d_val.as<int32_t>(), symmetric,
                       (uint32_t *)nullptr, d_rptr.as<unsigned long long>(), d_cols.as<uint32_t>(), d_ed.as<int32_t>(), (unsigned long long *)nullptr);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    ISO_HIP_CHECK(copy_d2h(out_cols, d_cols.p, n_edges * 4));
    ISO_HIP_CHECK(copy_d2h(out_ed, d_ed.p, n_edges * 4));
    clk.lap("hwg: edges");
    if (kernel_ms) *kernel_ms = tm.total + ms_rows;
    return ISOCON_OK;
}
