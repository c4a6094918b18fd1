// nn_context.inc -- state and helpers of the nearest-neighbour search on the host (first of the nn_*.inc pieces included by isocon_hip.hip:
// nn_context / nn_bounds / nn_lists / nn_main / nn_wide / nn_images / nn_entry -- one translation unit, split by phase).
//
// Phase A (nn_main.inc): every admissible pair within |len difference| <= 63 through the 64-row band.  Ordinarily: q-gram bounds of every
//          pair of the pass (k_qgram_mm), the pairs with the smallest bounds aligned first as seeds (k_ed_lanes), the survivors of the
//          bounds as lists through the block filter, then 64-row and 32-row table launches (k_nn_scan_refill) for the entries with
//          enough pairs and one pair per lane (k_ed_lanes) for the rest.  Reads against many candidates (2-set) go the same way.
//          Fallbacks: the refill kernel by its own admission when bounds or lists are not affordable; k_nn_scan_lds / k_nn_scan_up
//          when its table does not fit the LDS (or under nn_tiles); explicit tiles (k_nn_tiles, the candidate as the shared sequence)
//          for reads against few candidates.
// Phase B (nn_wide.inc): queries that still have no neighbour (NN distance > 63): 128- to 512-row bands over their whole admissible
//          window, the band chosen from a sample, then the un-banded kernel with k = len(query) (the reference's "best_ed = len(seq1)",
//          modules/nearest_neighbor_graph.py:129).

namespace {

struct HostClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    const bool on = getenv("ISOCON_DEBUG") != nullptr;
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[isocon] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

struct NNContext {
    isocon_store *st = nullptr;
    uint32_t n = 0;
    std::vector<uint8_t> qflag, tflag;
    bool two_set = false;
    bool depth_binds = false;            // 2-set: neighbor_search_depth is smaller than the number of targets
    std::vector<uint8_t> wide_mask;      // phase B in sub-steps (sharded callers): the queries of the whole phase, fixed at its start (empty: derived from best[])
    int32_t min_d = 1;
    uint32_t depth = 0x7fffffffu;
    DevBuf d_best, d_qf, d_tf, d_hits, d_hit_count, d_stats;   // bound to the store's scratch pool in nn_setup
    DevBuf d_text;                 // nibble store of the lane-refill kernels (built on first use)
    uint32_t text_stride = 0;
    bool text_ready = false;
    DevBuf d_qprof, d_qsum, d_lb;   // q-gram profiles and the bound matrix of the main pass (qgram_mm.hpp)
    DevBuf d_chunks;       // tile table of k_qgram_mm, with the matrix' row offsets and row lengths behind it (one buffer: one upload)
    const unsigned long long *lb_row_dev = nullptr;
    const uint32_t *lb_len_dev = nullptr;
    DevBuf d_lbt, d_offT, d_sloT, d_lenT, d_score;     // the transposed matrix, its row layout and the entries' hub scores
    DevBuf d_order;        // launch slots of the main pass, widest window first
    DevBuf d_rowmin, d_colmin, d_seed_a, d_seed_b, d_seed_n;   // smallest bounds per row / column, the seed pairs made of them and their number
    uint64_t hits_cap = 0;
    std::vector<int32_t> best;   // host mirror
    std::vector<int32_t> hits;   // host triples
    isocon_nn_stats stats;
    EventTimer tm;

    // free device memory, asked for once per entry point (the pool only grows: what a later phase finds can only be less by what an
    // earlier one took, and every check below leaves half of it alone)
    size_t free_bytes = 0;
    int free_state = 0;          // 0: not asked yet, 1: known, -1: the query failed
    bool free_mem(size_t &free_b)
    {
        if (free_state == 0) {
            size_t total_b = 0;
            free_state = hipMemGetInfo(&free_bytes, &total_b) == hipSuccess ? 1 : -1;
            if (free_state < 0) (void)hipGetLastError();
        }
        free_b = free_bytes;
        return free_state > 0;
    }
    // nibble rows padded to the longest sequence, in two steps: text_affordable() -- false if there is no room for them (callers fall
    // back to other kernels) -- and build_text(), immediately before the first launch that reads them (a call whose survivors all go
    // to the pair-per-lane kernel never writes them).
    bool text_room = false;
    bool text_affordable()
    {
        if (text_ready || text_room) return true;
        text_stride = (uint32_t)NN_TEXT_PAD_FRONT + (uint32_t)((st->maxlen + 7) / 8) + (uint32_t)NN_TEXT_PAD_BACK;
        size_t free_b = 0;
        if (!free_mem(free_b) || (size_t)n * text_stride * 4 > free_b / 2) return false;
        d_text.pool = &st->pool;
        d_text.slot = SLOT_NN_IL;
        if (d_text.alloc((size_t)std::max<uint32_t>(n, 1) * text_stride * 4) != ISOCON_OK) return false;
        text_room = true;
        return true;
    }
    bool build_text()
    {
        if (text_ready) return true;
        if (!text_room) return false;
        hipLaunchKernelGGL(k_build_nibble_text, dim3(std::max<uint32_t>(n, 1)), dim3(256), 0, 0, st->dev, d_text.as<uint32_t>(), text_stride);
        if (hipGetLastError() != hipSuccess) { g_last_error = "k_build_nibble_text: launch failed"; return false; }
        text_ready = true;
        return true;
    }
    bool ensure_text() { return text_affordable() && build_text(); }
    // 2-bit texts of the block filter (nn_filter.hpp).  A step that builds its bounds has them written by the profile kernel
    // (build_bounds asks filter_wanted() and text2_room() and sets text2_ready); a call that finds its bound matrix in the pool
    // (bound_tag: no profile kernel runs) builds them here on first use.
    DevBuf d_text2;
    uint32_t text2_stride = 0;
    bool text2_ready = false;
    bool filter_wanted() const { return !variant("nn_no_block_filter") && !variant("nn_no_list") && st->maxlen < 16384; }          // (what plan_lists asks in front of the filter)
    bool text2_room()
    {
        if (d_text2.p) return true;
        text2_stride = nnf_text2_stride(st->maxlen);
        size_t free_b = 0;
        if (!free_mem(free_b) || (size_t)n * text2_stride * 4 > free_b / 2 + st->pool.slots[SLOT_NN_TEXT2].cap) return false;
        d_text2.pool = &st->pool;
        d_text2.slot = SLOT_NN_TEXT2;
        if (d_text2.alloc((size_t)std::max<uint32_t>(n, 1) * text2_stride * 4) != ISOCON_OK) { d_text2.p = nullptr; return false; }
        return true;
    }
    bool ensure_text2()
    {
        if (text2_ready) return true;
        if (!text2_room()) return false;
        hipLaunchKernelGGL(k_build_text2, dim3(std::max<uint32_t>(n, 1)), dim3(256), 0, 0, st->dev, d_text2.as<uint32_t>(), text2_stride);
        if (hipGetLastError() != hipSuccess) return false;
        text2_ready = true;
        return true;
    }
    // Lower bounds for the pairs (q, p), q = Q.entry(s) (common.hpp), q < p, len(p) - len(q) <= kcap, p - q <= depth, in the row
    // layout of the main pass (P.lb, P.lb_row).  Leaves P.lb == nullptr when the matrix is not affordable (the pass then aligns
    // every pair, as it did before the bounds existed).
    // Widest windows first pays when a launch is only a few rounds of workgroups (a rank's share of a sharded search: 10.4 -> 7.5 ms
    // for 6 250 entries of C3); on long launches index order wins by 3 % (neighbouring entries share their lanes' texts in L2).
    static bool use_slot_order(uint32_t nq)
    {
        if (const char *e = variant_value("nn_order")) return atoi(e) != 0;
        return nq <= 16384;
    }
    // q-gram profiles, the bound matrix of the shard and its transposed copy: nn_bounds.inc
    int build_bounds(const QMap &Q, int32_t kcap, NNParams &P, bool want_seeds = false);
    std::vector<unsigned long long> lb_off_host;     // row layout of the last build_bounds (isocon_qgram_bound_matrix reads the matrix back)
    std::vector<uint32_t> lb_len_host;
    unsigned long long lb_total = 0;
    bool seeds_ready = false;
    uint32_t seed_nq = 0;
    int run_bound_seeds(const QMap &Q);          // nn_bounds.inc: propose_bound_seeds, then align_bound_seeds
    int propose_bound_seeds(const QMap &Q, uint32_t *classes_used = nullptr);
    int align_bound_seeds();
    // The table of the seed pairs (NNSeedKnown, nn_list.hpp): known_ready from the launch of THIS pass' seed pairs (run_bound_seeds) to the
    // next start of a pass (begin_pass: best[] is uploaded again, the hit list starts over) -- never across calls.  The kernels that make
    // flat pairs get it only where its argument holds as it is written down: one set with every entry query and target, thresholds that
    // tighten, the sequences themselves (not their images).
    DevBuf d_known;
    bool known_ready = false;
    static int seed_skip_mode()          // 1: settled pairs are not aligned again; 0: they are only counted (nn_seed_skip=0 / =count: A/B runs, tests)
    {
        const char *e = variant_value("nn_seed_skip");
        return e && (!strcmp(e, "0") || !strcmp(e, "count")) ? 0 : 1;
    }
    NNSeedKnown seed_known() const
    {
        if (!known_ready || !roles_uniform || fixed || image_pass || st->n_exc) return NNSeedKnown{nullptr, 0u};
        return NNSeedKnown{static_cast<const uint32_t *>(d_known.p), (uint32_t)seed_skip_mode()};
    }
    // The survivors of the bounds as lists (nn_list.hpp).  listed = false when the lists are not affordable or the bounds reject too
    // little (the caller then launches the kernel with its own admission).
    DevBuf d_ltot, d_lchunks, d_list, d_lpa, d_lpb, d_lmeta, d_ltasks;
    // chunk tables (one allocation): the two classes (64-row, 32-row) as the list builder wrote them, as the block filter left them (the
    // same two when the filter is off), and room for the two sorted copies the table launches read
    struct ListPlan {
        bool listed = false;
        unsigned long long n_chunks = 0, n_chunks_narrow = 0, n_small = 0;
        unsigned long long seed_known = 0;          // settled pairs the list builder and the filter met (left out of the n_small flat pairs if `K.drop`)
        NNSeedKnown K = {nullptr, 0u};              // what the kernels of the plan got; k_nn_chunks_to_pairs gets the same
        unsigned long long conv_a = 0, conv_b = 0, conv_pairs = 0;          // chunks (per class) whose pairs the caller appends to the n_small flat pairs
        NNChunk *a = nullptr, *b = nullptr, *sorted_a = nullptr, *sorted_b = nullptr;
    };
    int plan_lists(const QMap &Q, uint32_t nq, const NNParams &PR, ListPlan &L);          // nn_lists.inc
    NNParams params(int32_t kcap)
    {
        NNParams P;
        P.best = d_best.as<int32_t>();
        P.qflag = d_qf.as<uint8_t>();
        P.tflag = d_tf.as<uint8_t>();
        P.hits = d_hits.as<int32_t>();
        P.hit_count = d_hit_count.as<unsigned long long>();
        P.stats = d_stats.as<unsigned long long>();
        P.hits_cap = hits_cap;
        P.kcap = kcap;
        P.min_d = image_pass ? 0 : min_d;          // (two different sequences can have the same image: distance 0 between images is a candidate)
        P.depth = depth;
        P.fixed = fixed ? 1 : 0;
        P.q_list = nullptr;
        P.own = QMap{0u, n, 1u, 0u};
        P.lb = nullptr;
        P.lb_row = nullptr;
        P.slot_order = nullptr;
        P.wg_base = 0;
        P.chunks = nullptr;
        P.list = nullptr;
        return P;
    }

    // fill_best: the caller gave no bounds and the host mirror still holds NN_INF everywhere -- the next upload is a fill on the device
    // (isocon_nn_graph sets it in front of the 64-row phase; one upload consumes it)
    bool fill_best = false;
    bool best_on_host = true;          // false: a phase left its bounds on the device only (isocon_nn_graph fetches them with the CSR)
    int upload_best()
    {
        if (fill_best) {
            fill_best = false;
            if (n) ISO_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d_best.p, NN_INF, n, 0));
            return ISOCON_OK;
        }
        ISO_HIP_CHECK(copy_h2d(d_best.p, best.data(), (size_t)n * 4));
        return ISOCON_OK;
    }
    int download_best() { ISO_HIP_CHECK(copy_d2h(best.data(), d_best.p, (size_t)n * 4)); best_on_host = true; return ISOCON_OK; }
    // d_stats: two counter blocks -- [0] every launch but the 32-row table launch, [1] that one (nn_phase_a) -- and behind them the settled
    // pairs that k_nn_chunks_to_pairs met (nn_filter.hpp)
    static constexpr uint32_t KNOWN_COUNTER = 2 * (NN_COUNTER_SLOTS * 4 + 1);
    static constexpr uint32_t N_COUNTERS = KNOWN_COUNTER + 1;
    int reset_counters()
    {
        ISO_HIP_CHECK(hipMemsetAsync(d_hit_count.p, 0, 8, 0));
        ISO_HIP_CHECK(hipMemsetAsync(d_stats.p, 0, N_COUNTERS * 8, 0));
        return ISOCON_OK;
    }
    // Start of a pass of the 64-row phase: bounds, role flags (if nn_setup left them to this point) and counters.  The ordinary step --
    // constant roles, best[] a fill -- does all of it in one launch (k_nn_step_init) instead of five fills.
    int begin_pass()
    {
        known_ready = false;
        if (flags_deferred && fill_best && n) {
            flags_deferred = fill_best = false;
            hipLaunchKernelGGL(k_nn_step_init, dim3((std::max<uint32_t>(n, N_COUNTERS) + 255) / 256), dim3(256), 0, 0, d_best.as<int32_t>(), d_qf.as<uint8_t>(), d_tf.as<uint8_t>(), n,
                               (int32_t)NN_INF, d_hit_count.as<unsigned long long>(), d_stats.as<unsigned long long>(), N_COUNTERS);
            ISO_HIP_CHECK(hipGetLastError());
            return ISOCON_OK;
        }
        int rc;
        if ((rc = flush_flags()) || (rc = upload_best())) return rc;
        return reset_counters();
    }
    void add_counters(const unsigned long long *sc2)
    {
        for (int blk = 0; blk < 2; ++blk) {
            const unsigned long long *sc = sc2 + blk * (NN_COUNTER_SLOTS * 4 + 1);
            stats.pairs_prefiltered += sc[NN_COUNTER_SLOTS * 4];
            for (int i = 0; i < NN_COUNTER_SLOTS; ++i) {
                stats.pairs_evaluated += sc[i * 4 + 0];
                stats.cells_columns += sc[i * 4 + 1];
                stats.tiles += sc[i * 4 + 2];
                stats.live_columns += sc[i * 4 + 3];
                if (blk == 1) stats.narrow_columns += sc[i * 4 + 1];
            }
        }
        stats.pairs_seed_known += sc2[KNOWN_COUNTER];
        if (seed_skip_mode()) stats.pairs_lanes_aligned -= sc2[KNOWN_COUNTER];          // (run_listed_pass counted them as aligned: it only had the upper bound)
    }
    // pulls device hits into `out`; returns ISOCON_E_CAPACITY if the device list overflowed.  filter: drop on the device
    // every hit whose distance is above the endpoint's current best[] (it can never be part of the answer).
    // to_device: the (filtered) hits stay where they are -- dev_hits / dev_hit_count -- for a finalize that reads them there
    bool keep_dev = false;
    const int32_t *dev_hits = nullptr;
    uint64_t dev_hit_count = 0;
    int collect(std::vector<int32_t> &out, uint64_t *needed, bool filter = false, bool to_device = false)
    {
        unsigned long long cnt = 0;
        ISO_HIP_CHECK(memcpy_wait(&cnt, d_hit_count.p, 8, hipMemcpyDeviceToHost));
        unsigned long long sc2[N_COUNTERS];
        ISO_HIP_CHECK(memcpy_wait(sc2, d_stats.p, sizeof(sc2), hipMemcpyDeviceToHost));
        add_counters(sc2);
        if (needed) *needed = cnt;
        if (cnt > hits_cap) return ISOCON_E_CAPACITY;
        stats.hits += cnt;
        const void *src = d_hits.p;
        if (filter && cnt > 4096 && dev_hit_count == 0) {          // (the second list may hold an earlier pass' hits: then no filter)
            DevBuf d_h2(&st->pool, SLOT_NN_HITS2), d_c2(&st->pool, SLOT_NN_HITCOUNT2);
            int rc;
            if ((rc = d_h2.alloc((size_t)cnt * 12)) || (rc = d_c2.alloc(8))) return rc;
            ISO_HIP_CHECK(hipMemsetAsync(d_c2.p, 0, 8, 0));
            const unsigned blocks = (unsigned)std::min<unsigned long long>((cnt + 255) / 256, 4096);
            hipLaunchKernelGGL(k_filter_hits, dim3(blocks), dim3(256), 0, 0, d_hits.as<int32_t>(), cnt, d_best.as<int32_t>(), d_h2.as<int32_t>(),
                               d_c2.as<unsigned long long>());
            ISO_HIP_CHECK(hipGetLastError());
            ISO_HIP_CHECK(memcpy_wait(&cnt, d_c2.p, 8, hipMemcpyDeviceToHost));
            src = d_h2.p;
        }
        if (to_device) {
            dev_hits = static_cast<const int32_t *>(src);
            dev_hit_count = cnt;
            return ISOCON_OK;
        }
        const size_t base = out.size();
        out.resize(base + (size_t)cnt * 3);
        if (cnt) ISO_HIP_CHECK(copy_d2h(out.data() + base, src, (size_t)cnt * 12));
        return ISOCON_OK;
    }
    // The end of the 64-row phase when the CSR kernels follow on the device (csr_follows, set by isocon_nn_graph): the hit count, the
    // counters and "does the wide-band phase have to run" come back as ONE record; hits and bounds stay where they are.  The list is
    // not filtered: the CSR kernels keep exactly the hits that attain their endpoint's bound (nn_fin_valid), stale ones included or not.
    // The price is paid by the rare fallbacks -- phase B has to run, or a row is too long for the device sort: pull_dev_hits then brings
    // the unfiltered list to the host (several times the bytes k_filter_hits used to leave; nn_finalize_impl drops the stale hits itself).
    bool csr_follows = false;
    bool wide_needed = false;
    int collect_record(uint64_t *needed)
    {
        DevBuf d_rec(&st->pool, SLOT_NN_RECORD);
        int rc;
        if ((rc = d_rec.alloc((2 + N_COUNTERS) * 8))) return rc;
        ISO_HIP_CHECK(hipMemsetAsync(d_rec.p, 0, 16, 0));
        hipLaunchKernelGGL(k_nn_step_record, dim3(std::max<uint32_t>(1, (n + 255) / 256)), dim3(256), 0, 0, d_hit_count.as<unsigned long long>(), d_stats.as<unsigned long long>(),
                           N_COUNTERS, d_best.as<int32_t>(), d_qf.as<uint8_t>(), st->dev.lens, n, d_rec.as<unsigned long long>());
        ISO_HIP_CHECK(hipGetLastError());
        unsigned long long rec[2 + N_COUNTERS];
        ISO_HIP_CHECK(memcpy_wait(rec, d_rec.p, sizeof(rec), hipMemcpyDeviceToHost));
        add_counters(rec + 2);
        if (needed) *needed = rec[0];
        if (rec[0] > hits_cap) return ISOCON_E_CAPACITY;
        stats.hits += rec[0];
        wide_needed = rec[1] != 0;
        dev_hits = d_hits.as<int32_t>();
        dev_hit_count = rec[0];
        best_on_host = false;
        return ISOCON_OK;
    }
    // the hits a pass left on the device join the host list (before anything else writes to the device lists)
    int pull_dev_hits()
    {
        if (dev_hit_count) {
            const size_t base = hits.size();
            hits.resize(base + (size_t)dev_hit_count * 3);
            ISO_HIP_CHECK(copy_d2h(hits.data() + base, dev_hits, (size_t)dev_hit_count * 12));
        }
        dev_hits = nullptr;
        dev_hit_count = 0;
        return ISOCON_OK;
    }
    // Entries that hold symbols outside the planes' map (isocon_store::exc) carry no role on the DEVICE: no bit-vector kernel aligns a
    // pair of theirs.  Their pairs are aligned on the bytes (k_ed_bytes, through nn_phase_a_images / nn_phase_b_images in nn_images.inc) and applied with the host flags.
    bool is_exc(uint32_t q) const { return st->n_exc != 0 && st->exc[q] != 0; }
    bool mask_exc = true;          // exceptional entries carry no role on the device (false: the passes over the images, nn_phase_a_images)
    bool image_pass = false;       // the kernels compare images: min_d does not apply to their distances
    bool fixed = false;            // NNParams::fixed
    bool dev_excluded(uint32_t q) const { return mask_exc && is_exc(q); }
    bool flags_dirty = false;      // a wide stage left its own query flags on the device
    bool roles_uniform = false;    // 1-set, no converged entry: every entry is query and target
    // isocon_nn_graph: constant role flags are not filled by nn_setup but with the start of the first pass (begin_pass), or by
    // flush_flags() in front of anything else that reads them on the device
    bool defer_flags = false, flags_deferred = false;
    int flush_flags()
    {
        if (!flags_deferred) return ISOCON_OK;
        flags_deferred = false;
        ISO_HIP_CHECK(hipMemsetAsync(d_qf.p, 1, n, 0));
        ISO_HIP_CHECK(hipMemsetAsync(d_tf.p, 1, n, 0));
        return ISOCON_OK;
    }
    int upload_flags(bool fresh = false)
    {
        if (!n) return ISOCON_OK;
        flags_deferred = false;          // (whatever follows writes both arrays)
        if (fresh && roles_uniform && !st->n_exc) {          // (nn_setup: nothing to send, both role arrays are constants)
            if (defer_flags) { flags_deferred = true; return ISOCON_OK; }
            ISO_HIP_CHECK(hipMemsetAsync(d_qf.p, 1, n, 0));
            ISO_HIP_CHECK(hipMemsetAsync(d_tf.p, 1, n, 0));
            return ISOCON_OK;
        }
        if (!st->n_exc || !mask_exc) {
            ISO_HIP_CHECK(copy_h2d(d_qf.p, qflag.data(), n));
            ISO_HIP_CHECK(copy_h2d(d_tf.p, tflag.data(), n));
            return ISOCON_OK;
        }
        std::vector<uint8_t> q2(qflag), t2(tflag);
        for (uint32_t i = 0; i < n; ++i)
            if (st->exc[i]) q2[i] = t2[i] = 0;
        ISO_HIP_CHECK(copy_h2d(d_qf.p, q2.data(), n));
        ISO_HIP_CHECK(copy_h2d(d_tf.p, t2.data(), n));
        return ISOCON_OK;
    }
    bool admissible(uint32_t x, uint32_t y) const { return qflag[x] && tflag[y]; }   // x queries y
    // host-side application of one exact distance (same rule as nn_process_tile)
    void apply(uint32_t s, uint32_t p, int32_t d)
    {
        if (d < min_d) return;
        const int32_t ls = st->lens[s], lp = st->lens[p];
        // (fixed: the bounds are thresholds of a collecting pass, every pair within them is wanted -- nothing is tightened)
        if (admissible(s, p) && d <= ls && d <= best[s]) { if (!fixed) best[s] = d; hits.push_back((int32_t)s); hits.push_back((int32_t)p); hits.push_back(d); }
        if (admissible(p, s) && d <= lp && d <= best[p]) { if (!fixed) best[p] = d; hits.push_back((int32_t)p); hits.push_back((int32_t)s); hits.push_back(d); }
    }
};

template <int W>
int launch_nn_tiles(NNContext &C, const std::vector<uint32_t> &ts, const std::vector<uint32_t> &ids, int32_t kcap, float *ms_out)
{
    const size_t nt = ts.size();
    if (!nt) return ISOCON_OK;
    DevBuf d_ts(&C.st->pool, SLOT_NN_TS), d_ids(&C.st->pool, SLOT_NN_IDS);
    int rc;
    if ((rc = d_ts.alloc(nt * 4)) || (rc = d_ids.alloc(nt * 64 * 4))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_ts.p, ts.data(), nt * 4));
    ISO_HIP_CHECK(copy_h2d(d_ids.p, ids.data(), nt * 64 * 4));
    C.tm.start();
    hipLaunchKernelGGL(k_nn_tiles<W>, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, 0, C.st->dev, C.params(kcap),
                       d_ts.as<uint32_t>(), d_ids.as<uint32_t>(), (uint32_t)nt);
    ISO_HIP_CHECK(hipGetLastError());
    const float ms = C.tm.stop();
    if (ms_out) *ms_out += ms;
    return ISOCON_OK;
}

int run_nn_tiles(int W, NNContext &C, const std::vector<uint32_t> &ts, const std::vector<uint32_t> &ids, float *ms_out)
{
    switch (W) {
    case 1: return launch_nn_tiles<1>(C, ts, ids, 63, ms_out);
    case 2: return launch_nn_tiles<2>(C, ts, ids, 127, ms_out);
    case 4: return launch_nn_tiles<4>(C, ts, ids, 255, ms_out);
    case 8: return launch_nn_tiles<8>(C, ts, ids, 511, ms_out);
    default: return ISOCON_E_ARG;
    }
}

void push_tiles(std::vector<uint32_t> &ts, std::vector<uint32_t> &ids, uint32_t shared, const std::vector<uint32_t> &lanes)
{
    for (size_t i = 0; i < lanes.size(); i += 64) {
        ts.push_back(shared);
        for (size_t l = 0; l < 64; ++l) ids.push_back(i + l < lanes.size() ? lanes[i + l] : 0xffffffffu);
    }
}

// positions whose length is within `w` of len[x] (lens ascend)
void length_window(const std::vector<int32_t> &lens, uint32_t x, int32_t w, uint32_t &lo, uint32_t &hi)
{
    const int32_t L = lens[x];
    lo = (uint32_t)(std::lower_bound(lens.begin(), lens.end(), L - w) - lens.begin());
    hi = (uint32_t)(std::upper_bound(lens.begin(), lens.end(), L + w) - lens.begin());   // exclusive
}

int nn_setup(NNContext &C, isocon_store *s, const uint8_t *is_converged, const uint8_t *is_target, uint64_t depth,
             const int32_t *best_in, bool depth_walk = false)
{
    C.st = s;
    C.n = s->dev.n;
    C.d_best.pool = C.d_qf.pool = C.d_tf.pool = C.d_hits.pool = C.d_hit_count.pool = C.d_stats.pool = &s->pool;
    C.d_best.slot = SLOT_NN_BEST; C.d_qf.slot = SLOT_NN_QF; C.d_tf.slot = SLOT_NN_TF; C.d_hits.slot = SLOT_NN_HITS;
    C.d_hit_count.slot = SLOT_NN_HITCOUNT; C.d_stats.slot = SLOT_NN_STATS;
    const uint32_t n = C.n;
    for (uint32_t i = 1; i < n; ++i)
        if (s->lens[i] < s->lens[i - 1]) { g_last_error = "nearest-neighbour entry points need a length-sorted store"; return ISOCON_E_ARG; }
    C.two_set = is_target != nullptr;
    C.min_d = C.two_set ? 0 : 1;
    C.qflag.assign(n, 0);
    C.tflag.assign(n, 0);
    uint64_t n_targets = 0, n_converged = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (C.two_set) { C.tflag[i] = is_target[i] ? 1 : 0; C.qflag[i] = is_target[i] ? 0 : 1; n_targets += C.tflag[i]; }
        else { C.tflag[i] = 1; C.qflag[i] = (is_converged && is_converged[i]) ? 0 : 1; n_converged += C.qflag[i] == 0; }
    }
    C.roles_uniform = !C.two_set && n_converged == 0;          // (the wrappers always pass is_converged: mostly all zero)
    if (C.two_set) {
        // NNG:416 stops after `depth` candidate alignments (an order-dependent rule): the passes of this context are exact only when it
        // cannot bind.  depth_walk: the caller (isocon_nn_graph) sends such a call through nn2_depth_graph, which carries the rule out.
        C.depth_binds = depth < n_targets;
        if (C.depth_binds && !depth_walk) { g_last_error = "2-set search with neighbor_search_depth < number of targets is not supported"; return ISOCON_E_UNSUPPORTED; }
        C.depth = 0x7fffffffu;
    } else {
        if (depth == 0) { g_last_error = "neighbor_search_depth must be >= 1"; return ISOCON_E_ARG; }
        C.depth = depth > 0x7fffffffull ? 0x7fffffffu : (uint32_t)depth;
    }
    HostClock clk;
    C.best.assign(std::max<uint32_t>(n, 1), NN_INF);
    if (best_in) std::copy(best_in, best_in + n, C.best.begin());
    clk.lap("setup: host arrays");
    memset(&C.stats, 0, sizeof(C.stats));
    // every improvement of a bound is a hit (stale ones are filtered on the device afterwards): ~12 per entry at 50 k
    // reads, more on denser sets.  An overflow costs a second run (see nn_phase_a), so be generous: 12 B per slot.
    C.hits_cap = ((uint64_t)1 << 20) + (uint64_t)n * 48;
    if (const char *e = variant_value("hits_cap")) C.hits_cap = std::max<uint64_t>(16, strtoull(e, nullptr, 10));     // tests: force the overflow path
    int rc;
    if ((rc = C.d_best.alloc((size_t)std::max<uint32_t>(n, 1) * 4)) || (rc = C.d_qf.alloc(std::max<uint32_t>(n, 1))) ||
        (rc = C.d_tf.alloc(std::max<uint32_t>(n, 1))) || (rc = C.d_hits.alloc(C.hits_cap * 12)) || (rc = C.d_hit_count.alloc(8)) ||
        (rc = C.d_stats.alloc(NNContext::N_COUNTERS * 8)))
        return rc;
    clk.lap("setup: pool");
    if ((rc = C.upload_flags(true))) return rc;
    clk.lap("setup: role flags");
    return ISOCON_OK;
}

// the ABI's (q_begin, q_end, q_stride, q_block) as a QMap: q_block a power of two, 1 <= q_block <= q_stride
bool qmap_args_ok(uint32_t q_stride, uint32_t q_block) { return q_stride != 0 && q_block != 0 && (q_block & (q_block - 1)) == 0 && q_block <= q_stride; }
QMap qmap_of(uint32_t q_begin, uint32_t q_end, uint32_t q_stride, uint32_t q_block)
{
    uint32_t lg = 0;
    while ((1u << lg) < q_block) ++lg;
    return QMap{q_begin, q_end, q_stride, lg};
}

}  // namespace
