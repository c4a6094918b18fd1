// nn_wide.inc -- the wide-band phase: 128- to 512-row lane-refill launches over sampled band widths, then the un-banded kernel (included by isocon_hip.hip behind nn_context.inc).

namespace {

static constexpr uint32_t NN_WIDE_WG_PER_LAUNCH = 8192;

template <int W>
void launch_scan_wide(NNContext &C, const QMap &Q, int32_t kcap, const uint32_t *d_q_list = nullptr, uint32_t n_list = 0)
{
    const uint32_t nq = Q.count();
    // lane-refill kernel with the entry's match-mask planes in LDS when they fit, else the scalar-window scan
    const size_t lds_w = nn_refill_lds(C.st->maxlen, 64 * W);
    // waves per workgroup: 16, but 12 for the 512-row form -- its column loop needs 131 registers, three more than a 1 024-thread workgroup
    // leaves a wave (they were 16 B of scratch around the refill path); at 768 threads the budget is 168
    constexpr int NW = W == 8 ? 12 : 16;
    // d_q_list != nullptr: the "sparse" launch of k_nn_scan_refill (nn.hpp) -- one workgroup per listed query instead of one per
    // entry; pays when few entries act as queries (a workgroup per entry would run with one or two live lanes).
    if (!variant("nn_tiles") && nn_refill_fits(C.st->maxlen, 64 * W, NW) && C.st->maxlen < 16384 && C.n < (1u << 30) && C.ensure_text()) {
        if (hipFuncSetAttribute((const void *)k_nn_scan_refill<NW, W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w) == hipSuccess) {
            NNParams P = C.params(kcap);
            // A wide-band pass over many queries runs for seconds (C5, 200 000 reads, 384-row band: 45 s): it is issued as launches of at most
            // NN_WIDE_WG_PER_LAUNCH workgroups (<= ~2 s each at that size), so that the device is never held by one uninterruptible launch and a
            // rank's share has a unit.  The launches follow each other on the stream; thresholds carry over through best[].
            const uint32_t total = d_q_list ? n_list : nq;
            uint32_t per_launch = NN_WIDE_WG_PER_LAUNCH;
            if (const char *e = variant_value("nn_wide_per_launch")) per_launch = (uint32_t)std::max(1, atoi(e));      // tests: many launches on a small set
            for (uint32_t base = 0; base < total; base += per_launch) {
                const uint32_t cnt = std::min(per_launch, total - base);
                P.wg_base = base;
                if (d_q_list) {
                    P.q_list = d_q_list; P.own = Q;
                    hipLaunchKernelGGL((k_nn_scan_refill<NW, W>), dim3(cnt), dim3(NW * 64), lds_w, 0, C.st->dev, P, C.d_text.as<uint32_t>(), C.text_stride,
                                       QMap{0u, C.n, 1u, 0u}, 0);
                } else {
                    hipLaunchKernelGGL((k_nn_scan_refill<NW, W>), dim3(cnt), dim3(NW * 64), lds_w, 0, C.st->dev, P, C.d_text.as<uint32_t>(), C.text_stride,
                                       Q, 0);
                }
                C.stats.scan_launches += 1;
            }
            return;
        }
        (void)hipGetLastError();
    }
    // (scalar-window scan: instantiated for 128, 256 and 512 rows; a narrower cap inside a wider window is fine)
    constexpr int WS = W <= 2 ? 2 : W <= 4 ? 4 : 8;
    hipLaunchKernelGGL(k_nn_scan_up<WS>, dim3(nq), dim3(256), 0, 0, C.st->dev, C.params(kcap), Q, 0, 0x7fffffff, 4);
}

// One wide-band stage: the entries flagged in `flags` act as queries against everything with a 64 W-row band (k <= 64 W - 1); thresholds
// come from best[] (tightened by the kernels, or -- NNContext::fixed -- left as they are while every pair within them is recorded).
int nn_wide_stage(NNContext &C, const QMap &Q, int W, const std::vector<uint8_t> &flags, size_t count, const char *what)
{
    const uint32_t n = C.n;

    const int32_t kcap = 64 * W - 1;
    int rc;
    ISO_HIP_CHECK(copy_h2d(C.d_qf.p, flags.data(), n));
    C.flags_dirty = true;
    // few queries: one workgroup per query (both directions) instead of one per entry
    const bool sparse = count * 16 < n && C.depth >= n && !variant("nn_no_sparse");
    DevBuf d_list(&C.st->pool, SLOT_NN_PERM);
    std::vector<uint32_t> list;
    if (sparse) {
        for (uint32_t q = 0; q < n; ++q)
            if (flags[q]) list.push_back(q);
        if ((rc = d_list.alloc(std::max<size_t>(list.size(), 1) * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_list.p, list.data(), list.size() * 4));
    }
    const uint32_t *dl = sparse ? d_list.as<uint32_t>() : nullptr;
    const uint32_t nl = (uint32_t)list.size();
    for (;;) {
        if ((rc = C.upload_best()) || (rc = C.reset_counters())) return rc;
        C.tm.start();
        switch (W) {
        case 2: launch_scan_wide<2>(C, Q, kcap, dl, nl); break;
        case 3: launch_scan_wide<3>(C, Q, kcap, dl, nl); break;
        case 4: launch_scan_wide<4>(C, Q, kcap, dl, nl); break;
        case 5: launch_scan_wide<5>(C, Q, kcap, dl, nl); break;
        case 6: launch_scan_wide<6>(C, Q, kcap, dl, nl); break;
        case 7: launch_scan_wide<7>(C, Q, kcap, dl, nl); break;
        default: launch_scan_wide<8>(C, Q, kcap, dl, nl); break;
        }
        ISO_HIP_CHECK(hipGetLastError());
        const float wms = C.tm.stop();
        if (getenv("ISOCON_DEBUG")) fprintf(stderr, "[isocon] phaseB: %d-row band scan (%s%s), %zu queries: %.2f ms\n", 64 * W, what, sparse ? ", one workgroup per query" : "", count, wms);
        bool again = false;
        if ((rc = nn_end_pass(C, kcap, false, Regrouped(), nullptr, again))) return rc;          // (as in phase A: larger list, bounds kept)
        if (!again) return ISOCON_OK;
    }
}

// Phase B: entries that are still without a neighbour after the 64-row phase (NN distance > 63).
//   128/256/512-row bands: the same symmetric upward scan as phase A over the pairs whose LOWER index lies in
//   [q_begin, q_end), but only still-unresolved entries act as queries (device role flags), so a pair is aligned only
//   if it can matter; thresholds tighten through best[] exactly as in phase A.
//   Beyond 511: un-banded distances with k = len(query) for the owned unresolved queries (host pair list).
int nn_phase_b_planes(NNContext &C, const QMap &Q)
{
    const uint32_t q_begin = Q.begin, q_end = Q.end;
    const uint32_t n = C.n;
    const std::vector<int32_t> &lens = C.st->lens;
    if (q_begin >= q_end || n == 0) return ISOCON_OK;
    int32_t prevcap = 63;
    // unresolved ANYWHERE (a pair owned here may resolve an entry owned by another rank) ...
    // With a mask (a sharded caller runs the phase in sub-steps over sub-shards, reducing best[] in between): the phase's queries were
    // fixed when it began; one that has a bound from an earlier sub-step stays a query of every band that is wider than the bands it
    // cannot profit from any more -- its pairs of THIS sub-shard still have to be seen with k = its bound (ties included).
    const bool masked = !C.wide_mask.empty();
    auto unresolved_all = [&](int32_t cap_done) {
        std::vector<uint8_t> f(n, 0);
        size_t cnt = 0;
        for (uint32_t q = 0; q < n; ++q) {
            const bool open = masked ? (C.wide_mask[q] != 0 && (C.best[q] == NN_INF || C.best[q] > cap_done)) : C.best[q] == NN_INF;
            if (C.qflag[q] && open && lens[q] > cap_done && !C.dev_excluded(q)) { f[q] = 1; ++cnt; }
        }
        return std::make_pair(f, cnt);
    };
    C.flags_dirty = false;
    auto run_stage = [&](int W, const std::vector<uint8_t> &flags, size_t count, const char *what) -> int { return nn_wide_stage(C, Q, W, flags, count, what); };
    // Which band?  A column costs in proportion to the words of its band (~77 issue cycles per 64-row word, and the
    // narrower cap also prunes the length window: C5-shaped reads, 50 k: 512 rows 6.5 s, 448 rows 5.0 s, 384 rows 3.5 s), a
    // band that cannot succeed still costs most of its columns, and a query left over pays for all its pairs again.  So the
    // exact search runs first for a SAMPLE of ~128 unresolved entries (512 rows, a per cent of the work; only they act as
    // queries, so only their bounds move), and the band of the main stage is the narrowest that covers all but the largest
    // ~3 % of the sample's nearest-neighbour distances; the leftovers take 512 rows.  Few unresolved entries: 512 rows at once.
    bool first_stage = true;
    int prev_w = 1;
    for (;;) {
        auto uf = unresolved_all(prevcap);
        if (uf.second == 0) break;
        if (first_stage) {
            for (uint32_t sl = 0, nsl = Q.count(); sl < nsl; ++sl) C.stats.fallback_queries += uf.first[Q.entry(sl)];
        }
        int W = 8, rc;
        if (uf.second >= 2048 && prev_w < 7) {
            std::vector<uint8_t> sf(n, 0);
            std::vector<uint32_t> sample;
            const size_t stride = std::max<size_t>(1, uf.second / 128);
            size_t seen = 0;
            for (uint32_t q = 0; q < n; ++q)
                if (uf.first[q] && (seen++ % stride) == 0) { sf[q] = 1; sample.push_back(q); }
            if ((rc = run_stage(8, sf, sample.size(), "sample"))) return rc;
            std::vector<int32_t> dd;
            for (uint32_t q : sample)
                if (C.best[q] != NN_INF) dd.push_back(C.best[q]);
            if (dd.size() >= 16) {
                std::sort(dd.begin(), dd.end());
                const int32_t hi = dd[dd.size() - 1 - dd.size() / 32];
                W = prev_w + 1;
                while (W < 8 && hi > 64 * W - 1) ++W;
            }
            uf = unresolved_all(prevcap);
            if (uf.second == 0) break;
        }
        if (first_stage) { if (const char *e = variant_value("nn_first_w")) W = std::min(8, std::max(2, atoi(e))); }      // A/B runs
        first_stage = false;
        if ((rc = run_stage(W, uf.first, uf.second, "all unresolved"))) return rc;
        prevcap = 64 * W - 1;
        prev_w = W;
        if (W == 8) break;
    }
    if (C.flags_dirty) { int rc = C.upload_flags(); if (rc) return rc; C.flags_dirty = false; }
    // beyond 511: un-banded distances with k = len(query), owned queries only (single-rank callers own everything)
    std::vector<uint32_t> u;
    for (uint32_t sl = 0, nsl = Q.count(); sl < nsl; ++sl) {
        const uint32_t q = (uint32_t)Q.entry(sl);
        if (C.qflag[q] && C.best[q] == NN_INF && lens[q] > prevcap && (!masked || C.wide_mask[q]) && !C.dev_excluded(q)) u.push_back(q);
    }
    if (u.empty()) return ISOCON_OK;
    std::vector<uint32_t> pa, pb;
    std::vector<int32_t> pk;
    for (uint32_t q : u) {
        uint32_t lo, hi;
        length_window(lens, q, lens[q], lo, hi);
        if (!C.two_set) {
            const uint64_t dlo = q > C.depth ? q - C.depth : 0, dhi = std::min<uint64_t>((uint64_t)q + C.depth + 1, n);
            lo = std::max<uint32_t>(lo, (uint32_t)dlo);
            hi = std::min<uint32_t>(hi, (uint32_t)dhi);
        }
        for (uint32_t p = lo; p < hi; ++p)
            if (p != q && C.tflag[p] && !C.dev_excluded(p)) { pa.push_back(q); pb.push_back(p); pk.push_back(lens[q]); }
    }
    if (!pa.empty()) {
        std::vector<int32_t> dd(pa.size(), -1);
        float ems = 0.f;
        uint64_t fp = 0;
        int rc = ed_pairs_impl(C.st, pa.data(), pb.data(), pk.data(), pa.size(), dd.data(), &ems, &fp, C.image_pass);
        if (rc) return rc;
        C.tm.total += ems;
        C.stats.full_pairs += fp;
        if (getenv("ISOCON_DEBUG")) fprintf(stderr, "[isocon] phaseB: un-banded stage, %zu queries, %zu pairs (%llu through k_ed_full): %.2f ms\n", u.size(), pa.size(), (unsigned long long)fp, ems);
        for (size_t i = 0; i < pa.size(); ++i)
            if (dd[i] >= 0) {   // only the owned query's row is completed here (its partner may belong to another rank)
                const uint32_t q = pa[i], p = pb[i];
                const int32_t d = dd[i];
                if (d >= C.min_d && d <= lens[q] && d <= C.best[q]) { C.best[q] = d; C.hits.push_back((int32_t)q); C.hits.push_back((int32_t)p); C.hits.push_back(d); }
            }
    }
    return ISOCON_OK;
}

}  // namespace
