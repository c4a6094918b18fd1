// nn_entry.inc -- phase dispatch, the CSR on the device, and the C ABI entry points of the search (isocon_nn_graph, isocon_nn_partial*, isocon_nn_finalize*) (included by isocon_hip.hip behind nn_context.inc).

namespace {

int nn_phase_a(NNContext &C, const QMap &Q, bool allow_regroup = false, bool do_seed = true, bool do_main = true, bool seeded_before = false)
{
    if (!C.st->n_exc || !do_main) return nn_phase_a_planes(C, Q, allow_regroup, do_seed, do_main, seeded_before);
    return nn_phase_a_images(C, Q, allow_regroup, do_seed, seeded_before);
}

int nn_phase_b(NNContext &C, const QMap &Q)
{
    return C.st->n_exc ? nn_phase_b_images(C, Q) : nn_phase_b_planes(C, Q);
}


// blocking host waits of one entry point (isocon_nn_last_host_waits): counted from here to the end of the scope
struct WaitScope {
    isocon_store *s;
    explicit WaitScope(isocon_store *st) : s(st) { g_host_waits = 0; }
    ~WaitScope() { if (s) s->last_host_waits = g_host_waits; }
};

// The same CSR computed on the device (nn_finalize.hpp) from hits and bounds that are in device memory: seven small kernels, then one
// 16-byte record (row too long?  how many columns?) and ONE download of row pointers, bounds and columns, which sit behind one another
// in one buffer.  best_host = the same bounds on the host (for out_best), nullptr: they come back with the CSR.  Returns
// ISOCON_E_UNSUPPORTED when a row is too long for the per-thread sort (the caller then uses the host routine).
int nn_finalize_device_core(ScratchPool *pl, uint32_t n, const int32_t *d_best, const int32_t *best_host, const int32_t *d_hits, uint64_t n_hits,
                            int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap, uint64_t *n_cols_needed)
{
    DevBuf d_cnt(pl, SLOT_NN_FIN_CNT), d_start(pl, SLOT_NN_FIN_START), d_cur(pl, SLOT_NN_FIN_CUR), d_nb(pl, SLOT_NN_FIN_NB),
        d_len2(pl, SLOT_NN_FIN_LEN2), d_out(pl, SLOT_NN_FIN_OUT), d_rec(pl, SLOT_NN_FIN_FLAG);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "row pointers travel as they are");
    // [row_ptr: n + 1][best: n, only when the host does not have it][cols: up to n_hits], each part at a 16-byte boundary
    const size_t rp_bytes = (((size_t)n + 1) * 8 + 15) & ~(size_t)15, best_bytes = best_host ? 0 : ((size_t)n * 4 + 15) & ~(size_t)15;
    const size_t cols_off = rp_bytes + best_bytes;
    int rc;
    if ((rc = d_cnt.alloc((size_t)n * 4)) || (rc = d_start.alloc(((size_t)n + 1) * 8)) || (rc = d_cur.alloc((size_t)n * 4)) ||
        (rc = d_nb.alloc((size_t)n_hits * 4 + 16)) || (rc = d_len2.alloc((size_t)n * 4)) || (rc = d_out.alloc(cols_off + (size_t)n_hits * 4 + 16)) ||
        (rc = d_rec.alloc(16)))
        return rc;
    unsigned long long *d_rowptr = d_out.as<unsigned long long>();
    int32_t *d_best_out = best_host ? nullptr : reinterpret_cast<int32_t *>(d_out.as<char>() + rp_bytes);
    uint32_t *d_cols = reinterpret_cast<uint32_t *>(d_out.as<char>() + cols_off);
    ISO_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, (size_t)n * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_cur.p, 0, (size_t)n * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_rec.p, 0, 16, 0));
    const unsigned hb = (unsigned)std::max<uint64_t>(1, (n_hits + 255) / 256), nb_ = (n + 255) / 256;
    hipLaunchKernelGGL(k_fin_count, dim3(hb), dim3(256), 0, 0, d_hits, (unsigned long long)n_hits, d_best, n, d_cnt.as<uint32_t>());
    if ((rc = device_exscan<0, unsigned long long>(pl, d_cnt.as<uint32_t>(), n, d_start.as<unsigned long long>()))) return rc;
    hipLaunchKernelGGL(k_fin_scatter, dim3(hb), dim3(256), 0, 0, d_hits, (unsigned long long)n_hits, d_best, n,
                       d_start.as<unsigned long long>(), d_cur.as<uint32_t>(), d_nb.as<uint32_t>());
    hipLaunchKernelGGL(k_fin_rows, dim3(nb_), dim3(256), 0, 0, n, d_start.as<unsigned long long>(), d_nb.as<uint32_t>(), d_len2.as<uint32_t>(), d_rec.as<uint32_t>());
    if ((rc = device_exscan<0, unsigned long long>(pl, d_len2.as<uint32_t>(), n, d_rowptr))) return rc;
    hipLaunchKernelGGL(k_fin_gather, dim3(nb_), dim3(256), 0, 0, n, d_start.as<unsigned long long>(), d_nb.as<uint32_t>(), d_rowptr, d_cols);
    hipLaunchKernelGGL(k_fin_pack, dim3(std::max(1u, nb_)), dim3(256), 0, 0, n, d_rowptr, d_rec.as<unsigned long long>(), d_best, d_best_out);
    ISO_HIP_CHECK(hipGetLastError());
    unsigned long long rec[2] = {0, 0};          // {row too long (low word), columns}
    ISO_HIP_CHECK(memcpy_wait(rec, d_rec.p, sizeof(rec), hipMemcpyDeviceToHost));
    if (rec[0]) return ISOCON_E_UNSUPPORTED;
    const uint64_t total = rec[1];
    if (n_cols_needed) *n_cols_needed = total;
    if (total > cols_cap) return ISOCON_E_CAPACITY;
    const size_t bytes = cols_off + (size_t)total * 4;
    char *stg = bytes <= kStageBytes ? static_cast<char *>(g_stage.get(kStageBytes)) : nullptr;
    const int32_t *best_src = best_host;
    std::vector<int32_t> best_tmp;
    if (stg) {
        ISO_HIP_CHECK(memcpy_wait(stg, d_out.p, bytes, hipMemcpyDeviceToHost));
        memcpy(out_row_ptr, stg, ((size_t)n + 1) * 8);
        if (total) memcpy(out_cols, stg + cols_off, (size_t)total * 4);
        if (!best_src) best_src = reinterpret_cast<const int32_t *>(stg + rp_bytes);
    } else {          // larger than the staging buffer (or none): part by part
        ISO_HIP_CHECK(copy_d2h(out_row_ptr, d_rowptr, ((size_t)n + 1) * 8));
        if (total) ISO_HIP_CHECK(copy_d2h(out_cols, d_cols, (size_t)total * 4));
        if (!best_src) {
            best_tmp.resize(std::max<uint32_t>(n, 1));
            if (n) ISO_HIP_CHECK(copy_d2h(best_tmp.data(), d_best_out, (size_t)n * 4));
            best_src = best_tmp.data();
        }
    }
    for (uint32_t i = 0; i < n; ++i) out_best[i] = out_row_ptr[i + 1] > out_row_ptr[i] ? best_src[i] : -1;
    return ISOCON_OK;
}

// ... from hits and bounds on the host: they go up once (a few MB)
int nn_finalize_device(isocon_store *st, uint32_t n, const int32_t *best, const int32_t *hits, uint64_t n_hits, int32_t *out_best,
                       uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap, uint64_t *n_cols_needed)
{
    ScratchPool *pl = &st->pool;
    DevBuf d_hits(pl, SLOT_NN_FIN_HITS), d_best(pl, SLOT_NN_FIN_BEST);
    int rc;
    if ((rc = d_hits.alloc((size_t)n_hits * 12)) || (rc = d_best.alloc((size_t)n * 4))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_hits.p, hits, (size_t)n_hits * 12));
    ISO_HIP_CHECK(copy_h2d(d_best.p, best, (size_t)n * 4));
    return nn_finalize_device_core(pl, n, d_best.as<int32_t>(), best, d_hits.as<int32_t>(), n_hits, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
}

// the depth-limited reads x candidates search (nn2_depth.inc)
int nn2_depth_graph(NNContext &C, uint64_t depth, int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                    uint64_t *n_cols_needed, isocon_nn_stats *stats);


}  // namespace

extern "C" int isocon_nn_partial(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                                 uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, int32_t phase, int32_t *best_inout,
                                 int32_t *out_hits, uint64_t hits_cap, uint64_t *n_hits, isocon_nn_stats *stats, const uint8_t *wide_queries)
{
    if (!s || !best_inout || !n_hits || (hits_cap && !out_hits) || phase < 0 || phase > 3 || !qmap_args_ok(q_stride, q_block)) return ISOCON_E_ARG;
    const uint32_t n = s->dev.n;
    if (q_end > n) q_end = n;
    const QMap Q = qmap_of(q_begin, q_end, q_stride, q_block);
    WaitScope waits(s);
    NNContext C;
    int rc = nn_setup(C, s, is_converged, is_target, depth, best_inout);
    if (rc) return rc;
    if (phase == 2 && wide_queries) C.wide_mask.assign(wide_queries, wide_queries + n);
    rc = phase == 2 ? nn_phase_b(C, Q) : nn_phase_a(C, Q, false, phase == 0 || phase == 3, phase == 1 || phase == 3, phase == 1);
    if (rc) return rc;
    C.tm.resolve();
    C.stats.kernel_ms = C.tm.total; C.stats.narrow_kernel_ms = C.tm.marked_total;
    if (stats) *stats = C.stats;
    std::copy(C.best.begin(), C.best.begin() + n, best_inout);
    *n_hits = C.hits.size() / 3;
    if (*n_hits > hits_cap) return ISOCON_E_CAPACITY;
    if (!C.hits.empty()) memcpy(out_hits, C.hits.data(), C.hits.size() * 4);
    return ISOCON_OK;
}

extern "C" int isocon_nn_finalize(uint32_t n, const int32_t *best, const int32_t *hits, uint64_t n_hits,
                                  int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                                  uint64_t *n_cols_needed)
{
    if ((n && (!best || !out_best)) || !out_row_ptr || (n_hits && !hits) || (cols_cap && !out_cols)) return ISOCON_E_ARG;
    return nn_finalize_impl(n, best, hits, n_hits, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
}

// ---- the device-resident variants of the sharded protocol (bounds and hits never visit the host between the exchange steps) ----
extern "C" int isocon_nn_partial_dev(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                                     uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, int32_t phase, int32_t *best_inout_dev,
                                     int32_t keep_hits, uint64_t *n_hits_held, isocon_nn_stats *stats, const uint8_t *wide_queries)
{
    if (!s || !best_inout_dev || !n_hits_held || phase < 0 || phase > 3 || !qmap_args_ok(q_stride, q_block)) return ISOCON_E_ARG;
    const uint32_t n = s->dev.n;
    if (q_end > n) q_end = n;
    const QMap Q = qmap_of(q_begin, q_end, q_stride, q_block);
    WaitScope waits(s);
    std::vector<int32_t> best(std::max<uint32_t>(n, 1), NN_INF);
    if (n) ISO_HIP_CHECK(copy_d2h(best.data(), best_inout_dev, (size_t)n * 4));
    NNContext C;
    int rc = nn_setup(C, s, is_converged, is_target, depth, best.data());
    if (rc) return rc;
    if (phase == 2 && wide_queries) C.wide_mask.assign(wide_queries, wide_queries + n);
    C.keep_dev = phase != 2;          // the main pass' hits go from its device list to the held list without visiting the host
    rc = phase == 2 ? nn_phase_b(C, Q) : nn_phase_a(C, Q, false, phase == 0 || phase == 3, phase == 1 || phase == 3, phase == 1);
    if (rc) return rc;
    C.tm.resolve();
    C.stats.kernel_ms = C.tm.total; C.stats.narrow_kernel_ms = C.tm.marked_total;
    if (stats) *stats = C.stats;
    if (n) ISO_HIP_CHECK(copy_h2d(best_inout_dev, C.best.data(), (size_t)n * 4));
    if (!keep_hits || s->pool.held_hits.store_serial != s->serial) s->pool.held_hits = HeldHits{s->serial, 0};
    const uint64_t add_host = C.hits.size() / 3, add = add_host + C.dev_hit_count, have = s->pool.held_hits.rows;
    ScratchPool::Slot &slot = s->pool.slots[SLOT_NN_ACC_HITS];
    if ((have + add) * 12 > slot.cap) {          // grow, keeping what is held
        void *bigger = nullptr;
        const size_t want = (size_t)(have + add) * 12 * 2 + ((size_t)1 << 20);
        ISO_HIP_CHECK(hipMalloc(&bigger, want));
        if (have) ISO_HIP_CHECK(memcpy_wait(bigger, slot.p, (size_t)have * 12, hipMemcpyDeviceToDevice));
        if (slot.p) (void)hipFree(slot.p);
        slot.p = bigger; slot.cap = want;
    }
    if (add_host) ISO_HIP_CHECK(copy_h2d(static_cast<char *>(slot.p) + (size_t)have * 12, C.hits.data(), (size_t)add_host * 12));
    if (C.dev_hit_count)
        ISO_HIP_CHECK(memcpy_wait(static_cast<char *>(slot.p) + (size_t)(have + add_host) * 12, C.dev_hits, (size_t)C.dev_hit_count * 12, hipMemcpyDeviceToDevice));
    s->pool.held_hits.rows = have + add;
    *n_hits_held = s->pool.held_hits.rows;
    return ISOCON_OK;
}

extern "C" int isocon_nn_hits_dev(isocon_store *s, const int32_t *best_dev, int32_t *out_hits_dev, uint64_t cap_rows, uint64_t *n_kept)
{
    if (!s || !best_dev || (cap_rows && !out_hits_dev)) return ISOCON_E_ARG;
    uint64_t rows = s->pool.held_hits.store_serial == s->serial ? s->pool.held_hits.rows : 0;
    if (s->pool.slots[SLOT_NN_ACC_HITS].cap < rows * 12) rows = 0;          // (the scratch pool was released in between)
    if (rows > cap_rows) return ISOCON_E_CAPACITY;
    if (cap_rows) ISO_HIP_CHECK(hipMemsetAsync(out_hits_dev, 0xff, (size_t)cap_rows * 12, 0));          // unused rows: (-1, -1, -1)
    unsigned long long kept = 0;
    if (rows) {
        DevBuf d_c(&s->pool, SLOT_NN_HITCOUNT2);
        int rc;
        if ((rc = d_c.alloc(8))) return rc;
        ISO_HIP_CHECK(hipMemsetAsync(d_c.p, 0, 8, 0));
        const unsigned blocks = (unsigned)std::min<unsigned long long>((rows + 255) / 256, 4096);
        hipLaunchKernelGGL(k_filter_hits, dim3(blocks), dim3(256), 0, 0, static_cast<const int32_t *>(s->pool.slots[SLOT_NN_ACC_HITS].p), (unsigned long long)rows,
                           best_dev, out_hits_dev, d_c.as<unsigned long long>());
        ISO_HIP_CHECK(hipGetLastError());
        if (n_kept) ISO_HIP_CHECK(memcpy_wait(&kept, d_c.p, 8, hipMemcpyDeviceToHost));
    }
    if (n_kept) *n_kept = kept;
    return ISOCON_OK;
}

extern "C" int isocon_nn_finalize_dev(isocon_store *s, const int32_t *best_dev, const int32_t *hits_dev, uint64_t n_rows,
                                      int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap, uint64_t *n_cols_needed)
{
    if (!s || !out_row_ptr || (n_rows && !hits_dev) || (cols_cap && !out_cols)) return ISOCON_E_ARG;
    const uint32_t n = s->dev.n;
    if (n && (!best_dev || !out_best)) return ISOCON_E_ARG;
    std::vector<int32_t> best(std::max<uint32_t>(n, 1));
    if (n) ISO_HIP_CHECK(copy_d2h(best.data(), best_dev, (size_t)n * 4));
    int rc = nn_finalize_device_core(&s->pool, n, best_dev, best.data(), hits_dev, n_rows, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
    if (rc != ISOCON_E_UNSUPPORTED) return rc;
    std::vector<int32_t> hits((size_t)n_rows * 3);          // a row too long for the device sort: host routine
    if (n_rows) ISO_HIP_CHECK(copy_d2h(hits.data(), hits_dev, (size_t)n_rows * 12));
    return nn_finalize_impl(n, best.data(), hits.data(), n_rows, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
}

extern "C" int isocon_nn_graph(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                               int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                               uint64_t *n_cols_needed, isocon_nn_stats *stats)
{
    if (!s || !out_best || !out_row_ptr || (cols_cap && !out_cols)) return ISOCON_E_ARG;
    const uint32_t n = s->dev.n;
    HostClock clk0;
    if (getenv("ISOCON_DEBUG")) { (void)hipDeviceSynchronize(); clk0.lap("sync at entry"); }
    struct Total { std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
                   ~Total() { if (getenv("ISOCON_DEBUG")) fprintf(stderr, "[isocon] %-28s %8.2f ms\n", "isocon_nn_graph total", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count()); } } total;
    WaitScope waits(s);
    NNContext C;
    C.defer_flags = true;          // (constant role flags: filled with the start of the first pass, NNContext::begin_pass)
    int rc = nn_setup(C, s, is_converged, is_target, depth, nullptr, true);
    if (rc) return rc;
    clk0.lap("setup");
    if (getenv("ISOCON_DEBUG")) { (void)hipDeviceSynchronize(); clk0.lap("sync after setup"); }
    // 2-set with a depth limit that binds: the order-dependent rule of NNG:416, round by round (ISOCON_DEBUG_VARIANT=nn_2set_walk: every 2-set call)
    if (C.two_set && (C.depth_binds || variant("nn_2set_walk"))) return (rc = C.flush_flags()) ? rc : nn2_depth_graph(C, depth, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed, stats);
    C.keep_dev = n >= 1024 && !variant("nn_host_finalize");
    C.csr_follows = C.keep_dev;          // the ordinary case ends the 64-row phase with one record: hits and bounds stay on the device for the CSR kernels
    C.fill_best = !s->n_exc;             // no bounds from the caller: best[] starts as a fill on the device
    if ((rc = nn_phase_a(C, QMap{0u, n, 1u, 0u}, true, true, true))) return rc;
    HostClock clk;
    C.keep_dev = C.csr_follows = C.fill_best = false;
    bool run_b = true;
    if (!C.best_on_host) {
        // Phase A left hits and bounds on the device and said whether phase B is going to run -- an entry still without a neighbour that
        // the 64-row pass could not have resolved.  Phase B works on the host's bounds and appends to the device list from its start
        // again (and may re-allocate it): then both leave the device first.  Nothing to build a CSR from: the host routine takes over.
        if (C.wide_needed || !C.dev_hit_count) {
            if ((rc = C.download_best()) || (rc = C.pull_dev_hits())) return rc;
        } else run_b = false;
    }
    if (run_b && (rc = nn_phase_b(C, QMap{0u, n, 1u, 0u}))) return rc;
    clk.lap("phaseB");
    C.tm.resolve();
    if (C.dev_hit_count) {
        // phase A left its hits on the device.  Nothing came after it (the ordinary case): the CSR is built from them where they are.
        if (C.hits.empty()) {
            C.stats.kernel_ms = C.tm.total; C.stats.narrow_kernel_ms = C.tm.marked_total;
            if (stats) *stats = C.stats;
            rc = nn_finalize_device_core(&s->pool, n, C.d_best.as<int32_t>(), C.best_on_host ? C.best.data() : nullptr, C.dev_hits, C.dev_hit_count, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
            clk.lap("finalize (device hits)");
            if (rc != ISOCON_E_UNSUPPORTED && rc != ISOCON_E_HIP) return rc;
        }
        // ... otherwise (a row too long for the device sort) they join the host list, and the bounds the host's
        if (!C.best_on_host && (rc = C.download_best())) return rc;
        if ((rc = C.pull_dev_hits())) return rc;
    }
    C.stats.kernel_ms = C.tm.total; C.stats.narrow_kernel_ms = C.tm.marked_total;
    if (stats) *stats = C.stats;
    struct Lap { HostClock &c; ~Lap() { c.lap("finalize"); } } lap{clk};
    if (C.hits.size() / 3 >= 4096 && n >= 1024 && !variant("nn_host_finalize")) {
        rc = nn_finalize_device(s, n, C.best.data(), C.hits.data(), C.hits.size() / 3, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
        if (rc != ISOCON_E_UNSUPPORTED && rc != ISOCON_E_HIP) return rc;          // (a row too long for the device sort: host routine)
    }
    return nn_finalize_impl(n, C.best.data(), C.hits.data(), C.hits.size() / 3, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
}

// The bound matrix exactly as the main pass of a search over this shard consults it (every entry query and target), read back row
// by row: tests compare every byte with a restatement of the bound.
extern "C" int isocon_qgram_bound_matrix(isocon_store *s, uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block, uint64_t depth,
                                         uint64_t *out_row_ptr, uint8_t *out_bounds, uint64_t bounds_cap, uint64_t *n_bounds_needed)
{
    if (!s || !out_row_ptr || !qmap_args_ok(q_stride, q_block) || (bounds_cap && !out_bounds)) return ISOCON_E_ARG;
    if (s->n_exc) { g_last_error = "q-gram bounds are defined on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    if (q_end > n) q_end = n;
    NNContext C;
    int rc = nn_setup(C, s, nullptr, nullptr, depth, nullptr);
    if (rc) return rc;
    NNParams P = C.params(63);
    s->pool.bound_tag.valid = false;
    const QMap Q = qmap_of(q_begin, q_end, q_stride, q_block);
    const uint32_t nq = Q.count();
    if ((rc = C.build_bounds(Q, 63, P))) return rc;
    ISO_HIP_CHECK(device_wait());
    C.tm.resolve();
    s->pool.bound_tag.valid = false;
    uint64_t total = 0;
    if (P.lb == nullptr) {          // no pair inside the window (or no room for the matrix)
        for (uint32_t r = 0; r <= nq; ++r) out_row_ptr[r] = 0;
        if (n_bounds_needed) *n_bounds_needed = 0;
        bool any = false;
        for (uint32_t r = 0; r < C.lb_len_host.size(); ++r) any = any || C.lb_len_host[r] != 0;
        if (any) { g_last_error = "bound matrix not built (memory)"; return ISOCON_E_UNSUPPORTED; }
        return ISOCON_OK;
    }
    for (uint32_t r = 0; r < nq; ++r) { out_row_ptr[r] = total; total += C.lb_len_host[r]; }
    out_row_ptr[nq] = total;
    if (n_bounds_needed) *n_bounds_needed = total;
    if (total > bounds_cap) return ISOCON_E_CAPACITY;
    std::vector<uint8_t> raw((size_t)C.lb_total);
    ISO_HIP_CHECK(copy_d2h(raw.data(), P.lb, (size_t)C.lb_total));
    for (uint32_t r = 0; r < nq; ++r)
        if (C.lb_len_host[r]) memcpy(out_bounds + out_row_ptr[r], raw.data() + C.lb_off_host[r], C.lb_len_host[r]);
    // the transposed copy the list builder reads (nn_list.hpp) must hold the same bytes: row p, slot r <-> row r, column p
    if (C.d_lbt.p != nullptr) {
        std::vector<unsigned long long> offT(n);
        std::vector<uint32_t> sloT(n), lenT(n);
        ISO_HIP_CHECK(copy_d2h(offT.data(), C.d_offT.p, (size_t)n * 8));
        ISO_HIP_CHECK(copy_d2h(sloT.data(), C.d_sloT.p, (size_t)n * 4));
        ISO_HIP_CHECK(copy_d2h(lenT.data(), C.d_lenT.p, (size_t)n * 4));
        unsigned long long endT = 0, cells = 0;
        for (uint32_t p = 0; p < n; ++p) if (lenT[p]) endT = std::max(endT, offT[p] + lenT[p]);
        std::vector<uint8_t> rawT((size_t)endT + 1);
        if (endT) ISO_HIP_CHECK(copy_d2h(rawT.data(), C.d_lbt.p, (size_t)endT));
        for (uint32_t p = 0; p < n; ++p)
            for (uint32_t i = 0; i < lenT[p]; ++i) {
                const uint32_t r = sloT[p] + i;
                const uint64_t q = Q.entry(r);
                if (r >= nq || q >= p || p - q - 1 >= C.lb_len_host[r] || rawT[offT[p] + i] != raw[C.lb_off_host[r] + (p - q - 1)]) {
                    g_last_error = "transposed bound matrix differs from the matrix at entry " + std::to_string(p) + ", slot " + std::to_string(r);
                    return ISOCON_E_HIP;
                }
                ++cells;
            }
        if (cells != total) { g_last_error = "transposed bound matrix holds " + std::to_string(cells) + " cells, the matrix " + std::to_string(total); return ISOCON_E_HIP; }
    }
    return ISOCON_OK;
}


// What the epilogue of k_qgram_mm and k_qgram_seed_pairs leave beside the matrix for a search over this shard with these roles, read back
// raw: hub scores, row / column minima, the proposed seed pairs with their counter and the table of the seed pairs.  The launches are the
// search's own up to the proposal (NNContext::propose_bound_seeds); no pair is aligned.  Tests compare every word with a restatement.
extern "C" int isocon_qgram_seed_tables(isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
                                        uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block,
                                        uint32_t *out_score, uint64_t *out_rowmin, uint64_t *out_colmin, uint32_t *out_pa, uint32_t *out_pb,
                                        uint64_t *out_count, uint32_t *out_known, uint32_t *out_params)
{
    if (!s || !out_params || !qmap_args_ok(q_stride, q_block)) return ISOCON_E_ARG;
    out_params[0] = (uint32_t)QM_SEEDS; out_params[1] = QM_HUB_BOUND; out_params[2] = (uint32_t)QM_TILE; out_params[3] = 0u;
    const bool sizing = !out_score && !out_rowmin && !out_colmin && !out_pa && !out_pb && !out_count && !out_known;
    if (sizing) return ISOCON_OK;          // (the constants that size the arrays of the call proper)
    if (!out_score || !out_rowmin || !out_colmin || !out_pa || !out_pb || !out_count || !out_known) return ISOCON_E_ARG;
    if (s->n_exc) { g_last_error = "q-gram bounds are defined on the 2-bit planes: the set holds more than four distinct symbols"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    if (q_end > n) q_end = n;
    NNContext C;
    int rc = nn_setup(C, s, is_converged, is_target, depth, nullptr);
    if (rc) return rc;
    if ((rc = C.flush_flags())) return rc;          // (both role arrays are on the device before k_qgram_mm reads them)
    NNParams P = C.params(63);
    s->pool.bound_tag.valid = false;
    const QMap Q = qmap_of(q_begin, q_end, q_stride, q_block);
    const uint32_t nq = Q.count();
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the minima travel as they are");
    const size_t n_seed_words = (size_t)2 * QM_SEEDS * n;
    rc = C.build_bounds(Q, 63, P, true);
    s->pool.bound_tag.valid = false;
    if (rc) return rc;
    if (!C.seeds_ready) {
        // no pair inside the window: every table keeps its fill.  Anything else: no room for the matrix or for the minima.
        bool any = false;
        for (uint32_t r = 0; r < C.lb_len_host.size(); ++r) any = any || C.lb_len_host[r] != 0;
        if (any || P.lb != nullptr) { g_last_error = "seed tables not built (memory)"; return ISOCON_E_UNSUPPORTED; }
        ISO_HIP_CHECK(device_wait());
        C.tm.resolve();
        std::fill(out_score, out_score + n, 0u);
        std::fill(out_rowmin, out_rowmin + (size_t)nq * QM_SEEDS, ~(uint64_t)0);
        std::fill(out_colmin, out_colmin + (size_t)n * QM_SEEDS, ~(uint64_t)0);
        std::fill(out_pa, out_pa + n_seed_words, 0xffffffffu);
        std::fill(out_pb, out_pb + n_seed_words, 0xffffffffu);
        std::fill(out_known, out_known + (size_t)n * NN_KNOWN_SLOTS, 0xffffffffu);
        *out_count = 0;
        out_params[3] = (uint32_t)QM_SEEDS;
        return ISOCON_OK;
    }
    if (C.d_known.p == nullptr) { g_last_error = "no room for the table of the seed pairs"; return ISOCON_E_UNSUPPORTED; }
    C.tm.start();
    rc = C.propose_bound_seeds(Q, &out_params[3]);
    C.tm.stop_later(&C.stats.seed_kernel_ms);
    if (rc) return rc;
    ISO_HIP_CHECK(device_wait());
    C.tm.resolve();
    ISO_HIP_CHECK(copy_d2h(out_score, C.d_score.p, (size_t)n * 4));
    if (nq) ISO_HIP_CHECK(copy_d2h(out_rowmin, C.d_rowmin.p, (size_t)nq * QM_SEEDS * 8));
    ISO_HIP_CHECK(copy_d2h(out_colmin, C.d_colmin.p, (size_t)n * QM_SEEDS * 8));
    ISO_HIP_CHECK(copy_d2h(out_pa, C.d_seed_a.p, n_seed_words * 4));
    ISO_HIP_CHECK(copy_d2h(out_pb, C.d_seed_b.p, n_seed_words * 4));
    ISO_HIP_CHECK(copy_d2h(out_count, C.d_seed_n.p, 8));
    ISO_HIP_CHECK(copy_d2h(out_known, C.d_known.p, (size_t)n * NN_KNOWN_SLOTS * 4));
    return ISOCON_OK;
}
