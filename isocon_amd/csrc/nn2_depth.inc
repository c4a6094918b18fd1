// nn2_depth.inc -- host driver of the depth-limited reads x candidates search (kernels: nn2_depth.hpp, scheme: nn2_depth_core.hpp;
// included by isocon_hip.hip behind nn_entry's helpers).  isocon_nn_graph takes it for 2-set calls whose neighbor_search_depth is smaller
// than the number of targets, and for every 2-set call under ISOCON_DEBUG_VARIANT=nn_2set_walk.
//
// A round: k_nn2_speculate lists up to B + 1 pairs per open read in device memory, k_ed_lanes<false> decides the ones within 63 edits
// where they lie, the rest (thresholds above 63 -- the first rounds, k = len(read) -- and entries outside the planes' map) is compacted
// and goes through ed_pairs_impl, k_nn2_replay applies the reference rule.  B doubles from 1 to NN2_B_MAX: the first round's
// thresholds are whole read lengths, later rounds mostly run with the small best of a read that has found its candidate.

namespace {

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
    uint64_t pairs_total = 0, full_total = 0, wide_total = 0, bytes_total = 0;
    uint32_t rounds = 0;
    if (nq && nt) {
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
            if ((rc = d_pairs.alloc((size_t)cap * 20)) || (rc = d_wide.alloc((size_t)cap * 20))) return rc;
            NN2Pairs Q;
            Q.pa = d_pairs.as<uint32_t>(); Q.pb = Q.pa + cap; Q.pk = reinterpret_cast<int32_t *>(Q.pb + cap); Q.pk_lanes = Q.pk + cap; Q.pd = Q.pk_lanes + cap;
            Q.cap = cap;
            uint32_t *oa = d_wide.as<uint32_t>(), *ob = oa + cap, *oidx = ob + cap;
            int32_t *ok = reinterpret_cast<int32_t *>(oidx + cap), *ores = ok + cap;
            ISO_HIP_CHECK(hipMemsetAsync(ctr, 0, NN2_CTR_COUNT * 8, 0));
            C.tm.start();
            hipLaunchKernelGGL(k_nn2_speculate, dim3(qb), dim3(256), 0, 0, S, T, B, Q, exc, ctr);
            ISO_HIP_CHECK(hipGetLastError());
            C.tm.stop();
            ISO_HIP_CHECK(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
            if (hc[NN2_CTR_ERROR]) { g_last_error = "internal: depth-limited 2-set search listed more pairs than its round holds"; return ISOCON_E_HIP; }
            const uint64_t np = hc[NN2_CTR_PAIRS];
            if (np) {
                NNParams none;
                memset(&none, 0, sizeof(none));
                const unsigned pb_ = (unsigned)((np + 255) / 256);
                C.tm.start();
                hipLaunchKernelGGL(k_ed_lanes<false>, dim3(pb_), dim3(256), 0, 0, s->dev, none, Q.pa, Q.pb, Q.pk_lanes, (uint64_t)np, Q.pd);
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
    C.stats.full_pairs = full_total;
    C.stats.pairs_bytes = bytes_total;
    C.stats.scan_launches = rounds;
    C.stats.kernel_ms = C.tm.total;
    if (stats) *stats = C.stats;
    if (getenv("ISOCON_DEBUG")) fprintf(stderr, "[isocon] walk: %u rounds, %llu pairs, %llu beyond the 64-row band, %llu un-banded\n", rounds,
                                        (unsigned long long)pairs_total, (unsigned long long)wide_total, (unsigned long long)full_total);
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
