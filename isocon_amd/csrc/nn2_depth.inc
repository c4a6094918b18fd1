// nn2_depth.inc -- host driver of the depth-limited reads x candidates search (kernels: nn2_depth.hpp, scheme: nn2_depth_core.hpp;
// included by isocon_hip.hip behind nn_entry's helpers).  isocon_nn_graph takes it for 2-set calls whose neighbor_search_depth is smaller
// than the number of targets, and for every 2-set call under ISOCON_DEBUG_VARIANT=nn_2set_walk.
//
// A round: k_nn2_speculate lists up to B + 1 pairs per open read in device memory, k_ed_lanes<false> decides the ones within 63 edits
// where they lie, the rest (thresholds above 63 -- the first rounds, k = len(read) -- and entries outside the planes' map) is compacted
// and goes through ed_pairs_impl, k_nn2_replay applies the reference rule.  B doubles from 1 to NN2_B_MAX: the first round's
// thresholds are whole read lengths, later rounds mostly run with the small best of a read that has found its candidate.
//
// Under ISOCON_DEBUG_VARIANT=nn2_block_filter the block bound of nn_filter.hpp looks at the listed pairs between the listing and the
// 64-row kernel (k_nn2_block_reject): a pair with count > k is final with its -1 and is aligned by nobody; k_nn2_survivors makes the
// dense list the 64-row kernel runs on and k_nn2_scatter takes its distances back to the pairs' slots.  Rounds in which the test can
// reject nothing (the first: k = len(read)) make no task and run as before.  It is exact and rejects two thirds of the listed pairs at
// C3, but the 64-row kernel decides those pairs for less than the test costs, and the pairs that make the search slow (k = len(read),
// un-banded) cannot be rejected by a count: DESIGN.md 4.10, profiles/nn2set_depth.txt.  Hence off by default.

namespace {

// the test's probe stride: NN2_PROBE_STRIDE, or what ISOCON_DEBUG_VARIANT=nn2_probe_stride=2|4 says (A/B runs)
int nn2_probe_stride()
{
    if (const char *e = variant_value("nn2_probe_stride")) { const int v = atoi(e); if (v == 2 || v == 4) return v; }
    return NN2_PROBE_STRIDE;
}

hipError_t nn2_reject(int probe_stride, const uint32_t *text, uint32_t stride, const int32_t *lens, const NN2Task *tasks, unsigned long long n_tasks, const uint32_t *pb,
                      int32_t *pk_lanes, unsigned long long *ctr)
{
    return probe_stride == 4 ? nn2_launch_reject<4>(text, stride, lens, tasks, n_tasks, pb, pk_lanes, ctr)
                             : nn2_launch_reject<2>(text, stride, lens, tasks, n_tasks, pb, pk_lanes, ctr);
}

int nn2_depth_graph(NNContext &C, uint64_t depth, int32_t *out_best, uint64_t *out_row_ptr, uint32_t *out_cols, uint64_t cols_cap,
                    uint64_t *n_cols_needed, isocon_nn_stats *stats)
{
    isocon_store *s = C.st;
    ScratchPool *pl = &s->pool;
    const uint32_t n = C.n;
    HostClock clk;
    std::vector<uint32_t> tpos, qidx, tiq;
    for (uint32_t i = 0; i < n; ++i) {
        if (C.tflag[i]) tpos.push_back(i);
        else { qidx.push_back(i); tiq.push_back((uint32_t)tpos.size()); }
    }
    const uint32_t nq = (uint32_t)qidx.size(), nt = (uint32_t)tpos.size();
    for (uint32_t r = 0; r < nq; ++r) C.best[qidx[r]] = s->lens[qidx[r]];          // NNG:356 "best_ed = len(seq1)"
    int rc;
    if ((rc = C.upload_best()) || (rc = C.reset_counters())) return rc;
    uint64_t pairs_total = 0, full_total = 0, wide_total = 0, bytes_total = 0, rejected_total = 0, aligned_total = 0;
    uint32_t rounds = 0;
    if (nq && nt) {
        // the block test needs the 2-bit texts, built once per call; without room for them the walk aligns every pair it lists
        // (its launches, the text build included, are timed into filter_kernel_ms)
        // Off by default: measured, it costs more than it saves (profiles/nn2set_depth.txt); ISOCON_DEBUG_VARIANT=nn2_block_filter turns
        // it on, nn_no_block_filter -- the switch that means "run without the block filter" everywhere -- keeps it off.
        bool test = variant("nn2_block_filter") && !variant("nn_no_block_filter");
        if (test) {
            C.tm.start();
            test = C.ensure_text2();
            C.tm.stop_later(&C.stats.filter_kernel_ms);
        }
        const int probe_stride = nn2_probe_stride();
        // state of the reads: ten arrays of nq words (NN2State)
        DevBuf d_state(pl, SLOT_NN2_STATE), d_tpos(pl, SLOT_NN2_TPOS), d_exc(pl, SLOT_NN2_EXC), d_ctr(pl, SLOT_NN2_CTR), d_pairs(pl, SLOT_NN2_PAIRS),
            d_wide(pl, SLOT_NN2_WIDE);
        if ((rc = d_state.alloc((size_t)nq * 40)) || (rc = d_tpos.alloc((size_t)nt * 4)) || (rc = d_ctr.alloc(NN2_CTR_COUNT * 8))) return rc;
        {
            std::vector<uint32_t> init((size_t)nq * 10, 0u);
            std::copy(qidx.begin(), qidx.end(), init.begin());
            std::copy(tiq.begin(), tiq.end(), init.begin() + nq);
            for (uint32_t r = 0; r < nq; ++r) init[(size_t)4 * nq + r] = (uint32_t)s->lens[qidx[r]];
            ISO_HIP_CHECK(copy_h2d(d_state.p, init.data(), init.size() * 4));
            ISO_HIP_CHECK(copy_h2d(d_tpos.p, tpos.data(), (size_t)nt * 4));
        }
        const uint8_t *exc = nullptr;
        if (s->n_exc) {
            if ((rc = d_exc.alloc(n))) return rc;
            ISO_HIP_CHECK(copy_h2d(d_exc.p, s->exc.data(), n));
            exc = d_exc.as<uint8_t>();
        }
        uint32_t *w = d_state.as<uint32_t>();
        NN2State T;
        T.qidx = w; T.tiq = w + nq; T.a = w + 2 * (size_t)nq; T.b = w + 3 * (size_t)nq; T.best = reinterpret_cast<int32_t *>(w + 4 * (size_t)nq);
        T.processed = w + 5 * (size_t)nq; T.flags = w + 6 * (size_t)nq; T.jend = w + 7 * (size_t)nq; T.pbase = w + 8 * (size_t)nq; T.pcnt = w + 9 * (size_t)nq;
        T.nq = nq;
        const NN2Set S{s->d_lens, d_tpos.as<uint32_t>(), nt, depth > 0xffffffffull ? 0xffffffffu : (uint32_t)depth};
        unsigned long long *ctr = d_ctr.as<unsigned long long>();
        unsigned long long hc[NN2_CTR_COUNT];
        const unsigned qb = (nq + 255) / 256;
        uint64_t open = nq, dev_upper = 0;
        uint32_t B = 1;
        clk.lap("walk: setup");
        while (open) {
            // the pair arrays of the round and as many slots for the undecided ones: a read lists at most min(B, alignments the depth rule
            // still allows) + 1 pairs, so a small depth keeps the arrays small while B doubles (the pool's slots only grow)
            const uint64_t cap = open * (std::min<uint64_t>(B, std::max<uint64_t>(depth, 1)) + 1);
            if (cap > 0xffffffffull / 2) { g_last_error = "depth-limited 2-set search: more than 2^31 pairs in one round"; return ISOCON_E_UNSUPPORTED; }
            // ... and, for the block test, as many slots again for the pairs it leaves (sa, sb, sk, sidx, sd) and a task per open read
            const uint64_t tasks_cap = test ? open : 0;
            if ((rc = d_pairs.alloc((size_t)cap * (test ? 40 : 20) + (size_t)tasks_cap * sizeof(NN2Task))) || (rc = d_wide.alloc((size_t)cap * 20))) return rc;
            NN2Pairs Q;
            Q.pa = d_pairs.as<uint32_t>(); Q.pb = Q.pa + cap; Q.pk = reinterpret_cast<int32_t *>(Q.pb + cap); Q.pk_lanes = Q.pk + cap; Q.pd = Q.pk_lanes + cap;
            Q.cap = cap;
            uint32_t *sa = nullptr, *sb = nullptr, *sidx = nullptr;
            int32_t *sk = nullptr, *sd = nullptr;
            NN2Task *tasks = nullptr;
            if (test) {
                sa = reinterpret_cast<uint32_t *>(Q.pd + cap); sb = sa + cap; sidx = sb + cap;
                sk = reinterpret_cast<int32_t *>(sidx + cap); sd = sk + cap;
                tasks = reinterpret_cast<NN2Task *>(sd + cap);          // (40 cap bytes in: 8-byte aligned)
            }
            uint32_t *oa = d_wide.as<uint32_t>(), *ob = oa + cap, *oidx = ob + cap;
            int32_t *ok = reinterpret_cast<int32_t *>(oidx + cap), *ores = ok + cap;
            ISO_HIP_CHECK(hipMemsetAsync(ctr, 0, NN2_CTR_COUNT * 8, 0));
            C.tm.start();
            hipLaunchKernelGGL(k_nn2_speculate, dim3(qb), dim3(256), 0, 0, S, T, B, Q, exc, ctr, tasks, (unsigned long long)tasks_cap);
            ISO_HIP_CHECK(hipGetLastError());
            C.tm.stop();
            ISO_HIP_CHECK(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
            if (hc[NN2_CTR_ERROR]) { g_last_error = "internal: depth-limited 2-set search listed more pairs than its round holds"; return ISOCON_E_HIP; }
            const uint64_t np = hc[NN2_CTR_PAIRS];
            if (np) {
                NNParams none;
                memset(&none, 0, sizeof(none));
                const unsigned pb_ = (unsigned)((np + 255) / 256);
                // the block test, if the listing made tasks (their number came down with the round's first copy): the 64-row kernel then
                // runs on the dense list of the pairs it left -- as many as the device counted, at most np
                const unsigned long long n_tasks = std::min<unsigned long long>(hc[NN2_CTR_TASKS], tasks_cap);
                if (n_tasks) {
                    C.tm.start();
                    ISO_HIP_CHECK(nn2_reject(probe_stride, C.d_text2.as<uint32_t>(), C.text2_stride, s->dev.lens, tasks, n_tasks, Q.pb, Q.pk_lanes, ctr));
                    hipLaunchKernelGGL(k_nn2_survivors, dim3(pb_), dim3(256), 0, 0, Q, (unsigned long long)np, sa, sb, sk, sidx, ctr);
                    ISO_HIP_CHECK(hipGetLastError());
                    C.tm.stop_later(&C.stats.filter_kernel_ms);
                    C.tm.start();
                    hipLaunchKernelGGL(k_ed_lanes<false>, dim3(pb_), dim3(256), 0, 0, s->dev, none, sa, sb, sk, (uint64_t)np, sd, ctr + NN2_CTR_SURVIVORS);
                    ISO_HIP_CHECK(hipGetLastError());
                    C.tm.stop_later(nullptr);
                    C.tm.start();
                    hipLaunchKernelGGL(k_nn2_scatter, dim3(pb_), dim3(256), 0, 0, sidx, sd, (unsigned long long)np, (unsigned long long)np, Q.pd, ctr + NN2_CTR_SURVIVORS);
                    ISO_HIP_CHECK(hipGetLastError());
                    C.tm.stop_later(&C.stats.filter_kernel_ms);
                    C.tm.start();
                } else {
                    C.tm.start();
                    hipLaunchKernelGGL(k_ed_lanes<false>, dim3(pb_), dim3(256), 0, 0, s->dev, none, Q.pa, Q.pb, Q.pk_lanes, (uint64_t)np, Q.pd);
                }
                hipLaunchKernelGGL(k_nn2_undecided, dim3(pb_), dim3(256), 0, 0, Q, (unsigned long long)np, oa, ob, ok, oidx, ctr);
                ISO_HIP_CHECK(hipGetLastError());
                C.tm.stop();
                unsigned long long nw = 0;
                ISO_HIP_CHECK(hipMemcpy(&nw, ctr + NN2_CTR_WIDE, 8, hipMemcpyDeviceToHost));
                if (nw) {
                    std::vector<uint32_t> ha(nw), hb(nw);
                    std::vector<int32_t> hk(nw), res(nw, -1);
                    ISO_HIP_CHECK(copy_d2h(ha.data(), oa, (size_t)nw * 4));
                    ISO_HIP_CHECK(copy_d2h(hb.data(), ob, (size_t)nw * 4));
                    ISO_HIP_CHECK(copy_d2h(hk.data(), ok, (size_t)nw * 4));
                    float ms = 0.f;
                    uint64_t fp = 0;
                    if ((rc = ed_pairs_impl(s, ha.data(), hb.data(), hk.data(), nw, res.data(), &ms, &fp, false))) return rc;
                    C.tm.total += ms;
                    full_total += fp;
                    wide_total += nw;
                    ISO_HIP_CHECK(copy_h2d(ores, res.data(), (size_t)nw * 4));
                    C.tm.start();
                    hipLaunchKernelGGL(k_nn2_scatter, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, 0, oidx, ores, nw, (unsigned long long)np, Q.pd);
                    ISO_HIP_CHECK(hipGetLastError());
                    C.tm.stop();
                }
            }
            // a round records at most one hit per pair: when the device list could overflow, what it holds moves to the host first
            if (dev_upper + np > C.hits_cap) {
                if ((rc = C.collect(C.hits, nullptr))) return rc;
                ISO_HIP_CHECK(hipMemset(C.d_hit_count.p, 0, 8));
                dev_upper = 0;
            }
            dev_upper += np;
            C.tm.start();
            hipLaunchKernelGGL(k_nn2_replay, dim3(qb), dim3(256), 0, 0, S, T, Q, C.d_best.as<int32_t>(), C.d_hits.as<int32_t>(),
                               C.d_hit_count.as<unsigned long long>(), (unsigned long long)C.hits_cap, ctr);
            ISO_HIP_CHECK(hipGetLastError());
            C.tm.stop();
            ISO_HIP_CHECK(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
            if (hc[NN2_CTR_ERROR]) { g_last_error = "internal: depth-limited 2-set search visited a pair its round had not listed"; return ISOCON_E_HIP; }
            open = hc[NN2_CTR_OPEN];
            bytes_total += hc[NN2_CTR_BYTES];
            rejected_total += hc[NN2_CTR_REJECTED];
            aligned_total += np - hc[NN2_CTR_REJECTED];
            pairs_total += np;
            ++rounds;
            if (B < NN2_B_MAX) B *= 2;
        }
        clk.lap("walk: rounds");
    }
    if ((rc = C.download_best())) return rc;
    unsigned long long cnt = 0;
    ISO_HIP_CHECK(hipMemcpy(&cnt, C.d_hit_count.p, 8, hipMemcpyDeviceToHost));
    if (cnt > C.hits_cap) { g_last_error = "internal: depth-limited 2-set search overflowed its hit list"; return ISOCON_E_HIP; }
    C.stats.hits += cnt;
    C.stats.pairs_lanes = pairs_total;
    C.stats.pairs_block_rejected = rejected_total;
    C.stats.pairs_lanes_aligned = aligned_total;
    C.stats.full_pairs = full_total;
    C.stats.pairs_bytes = bytes_total;
    C.stats.scan_launches = rounds;
    C.stats.kernel_ms = C.tm.total;
    if (stats) *stats = C.stats;
    if (getenv("ISOCON_DEBUG")) fprintf(stderr, "[isocon] walk: %u rounds, %llu pairs, %llu rejected by the block bound, %llu beyond the 64-row band, %llu un-banded\n", rounds,
                                        (unsigned long long)pairs_total, (unsigned long long)rejected_total, (unsigned long long)wide_total, (unsigned long long)full_total);
    if (C.hits.empty() && n >= 1024 && !variant("nn_host_finalize")) {
        rc = nn_finalize_device_core(pl, n, C.d_best.as<int32_t>(), C.best.data(), C.d_hits.as<int32_t>(), cnt, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
        clk.lap("walk: finalize (device hits)");
        if (rc != ISOCON_E_UNSUPPORTED && rc != ISOCON_E_HIP) return rc;          // (a row too long for the device sort: host routine)
    }
    const size_t base = C.hits.size();
    C.hits.resize(base + (size_t)cnt * 3);
    if (cnt) ISO_HIP_CHECK(copy_d2h(C.hits.data() + base, C.d_hits.p, (size_t)cnt * 12));
    return nn_finalize_impl(n, C.best.data(), C.hits.data(), C.hits.size() / 3, out_best, out_row_ptr, out_cols, cols_cap, n_cols_needed);
}

}  // namespace

// ... exposed for tests: what the walk's block test decides on pairs the caller made.  The tasks are cut by the routine the listing
// kernel uses (nn2_cut_tasks) and the launch is the walk's own (nn2_reject); kernel_ms times that launch alone.
extern "C" int isocon_nn2_block_reject(isocon_store *s, const uint32_t *read, const uint32_t *target, const int32_t *k, uint64_t n_pairs, int32_t probe_stride,
                                       uint8_t *out_rejected, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (probe_stride != 4 && probe_stride != 2) return ISOCON_E_ARG;
    if (!s || (n_pairs && (!read || !target || !k || !out_rejected))) return ISOCON_E_ARG;
    if (!n_pairs) return ISOCON_OK;
    if (n_pairs >= ((uint64_t)1 << 31)) return ISOCON_E_ARG;
    const uint32_t n = s->dev.n;
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (read[p] >= n || target[p] >= n) { g_last_error = "pair index out of range"; return ISOCON_E_ARG; }
    // the threshold as the listing kernel writes it for the 64-row kernel: -1 for a pair with an entry outside the planes' map
    std::vector<int32_t> kl(n_pairs);
    for (uint64_t p = 0; p < n_pairs; ++p) kl[p] = (k[p] < 0 || s->is_exc(read[p]) || s->is_exc(target[p])) ? -1 : k[p];
    std::vector<NN2Task> tasks;
    nn2_cut_list(read, n_pairs, [&](unsigned long long p) { return nn2_tested(kl[p], s->lens[target[p]]); },
                 [&](uint32_t x, unsigned long long first, uint32_t pairs) { tasks.push_back(NN2Task{x, pairs, first}); });
    memset(out_rejected, 0, n_pairs);
    if (tasks.empty()) return ISOCON_OK;
    const uint32_t stride = nnf_text2_stride(s->maxlen);
    DevBuf d_text(&s->pool, SLOT_NN_TEXT2), d_b(&s->pool, SLOT_NN2_PAIRS), d_k(&s->pool, SLOT_NN2_WIDE), d_tasks(&s->pool, SLOT_NN2_STATE), d_ctr(&s->pool, SLOT_NN2_CTR);
    int rc;
    if ((rc = d_text.alloc((size_t)n * stride * 4)) || (rc = d_b.upload(target, n_pairs * 4)) || (rc = d_k.upload(kl.data(), n_pairs * 4)) ||
        (rc = d_tasks.upload(tasks.data(), tasks.size() * sizeof(NN2Task))) || (rc = d_ctr.alloc(NN2_CTR_COUNT * 8)))
        return rc;
    ISO_HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, NN2_CTR_COUNT * 8, 0));
    hipLaunchKernelGGL(k_build_text2, dim3(n), dim3(256), 0, 0, s->dev, d_text.as<uint32_t>(), stride);
    ISO_HIP_CHECK(hipGetLastError());
    EventTimer tm;
    tm.start();
    ISO_HIP_CHECK(nn2_reject(probe_stride, d_text.as<uint32_t>(), stride, s->dev.lens, d_tasks.as<NN2Task>(), tasks.size(), d_b.as<uint32_t>(), d_k.as<int32_t>(),
                             d_ctr.as<unsigned long long>()));
    const float ms = tm.stop();
    if (kernel_ms) *kernel_ms = ms;
    ISO_HIP_CHECK(copy_d2h(kl.data(), d_k.p, n_pairs * 4));
    for (uint64_t p = 0; p < n_pairs; ++p) out_rejected[p] = kl[p] == NN2_REJECTED;
    return ISOCON_OK;
}
