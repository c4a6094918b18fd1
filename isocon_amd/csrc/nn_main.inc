// nn_main.inc -- nn_phase_a_planes: the 64-row phase as a driver over its steps -- seeds, regrouping, the listed or unlisted main pass
// (or one of the two 2-set forms), the end of the pass (included by isocon_hip.hip behind nn_context.inc; launch shapes: nn_scan_shape.hpp).

namespace {

// The one place where (waves, half) becomes an instantiation of k_nn_scan_refill<NW, 1, HALF>: a 64-row (half: 32-row) launch of `grid`
// workgroups on the caller's store and nibble text.
template <int NW, bool HALF>
int launch_refill_as(NNContext &C, const NNRefillShape &sh, unsigned grid, const NNParams &P, const QMap &Q, int32_t first_tile)
{
    if (sh.raise_limit) ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<NW, 1, HALF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh.lds));
    hipLaunchKernelGGL((k_nn_scan_refill<NW, 1, HALF>), dim3(grid), dim3(NW * 64), sh.lds, 0, C.st->dev, P, C.d_text.as<uint32_t>(), C.text_stride, Q, first_tile);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

int launch_refill(NNContext &C, const NNRefillShape &sh, bool half, unsigned grid, const NNParams &P, const QMap &Q, int32_t first_tile)
{
    switch (sh.waves) {
    case 4: return half ? launch_refill_as<4, true>(C, sh, grid, P, Q, first_tile) : launch_refill_as<4, false>(C, sh, grid, P, Q, first_tile);
    case 8: return half ? launch_refill_as<8, true>(C, sh, grid, P, Q, first_tile) : launch_refill_as<8, false>(C, sh, grid, P, Q, first_tile);
    default: return half ? launch_refill_as<16, true>(C, sh, grid, P, Q, first_tile) : launch_refill_as<16, false>(C, sh, grid, P, Q, first_tile);
    }
}

// What the seed pass leaves when the main pass runs on a regrouped copy of the store (regroup_by_seed_hits); empty otherwise.
struct Regrouped {
    std::vector<uint32_t> perm;                          // position in the copy -> caller's position; empty: the store as it is
    std::vector<int32_t> seed_got;                       // the seed pass' hits, collected early (caller's positions)
    bool seed_collected = false;
    const std::vector<int32_t> *best_at_entry = nullptr; // bounds to start over from (a second run cannot keep bounds in permuted positions)
    const uint64_t *planes = nullptr;                    // the permuted planes

    // bounds and hits of the pass back to the caller's positions
    int unpermute(NNContext &C, std::vector<int32_t> &got) const
    {
        std::vector<int32_t> b(C.n);
        for (uint32_t i = 0; i < C.n; ++i) b[perm[i]] = C.best[i];
        std::copy(b.begin(), b.end(), C.best.begin());
        for (size_t i = 0; i + 2 < got.size(); i += 3) { got[i] = (int32_t)perm[got[i]]; got[i + 1] = (int32_t)perm[got[i + 1]]; }
        return C.upload_flags();
    }
};

// State of one pass of the 64-row phase (one turn of nn_phase_a_planes' retry loop).
struct PhaseAPass {
    bool do_seed, do_main, seeded_before;          // the caller's: which halves run, and whether an earlier call ran the seeds
    bool refill_main = false;                      // the lane-refill kernel can run the main pass (not nn_tiles, the table fits)
    bool bounds_wanted = false;
    NNParams PR;                                   // parameters of the main pass, with the bounds once they are built
    bool bound_seeded = false, bounds_built = false;
    bool seeds_clean;                              // the seeds ran only kernels that never emit "re-run" markers (a sharded call runs the seeds and
                                                   // the lists in separate phases: each is judged by what IT launched)
    bool no_markers = false;                       // so did the whole pass (survivor lists, bound seeds)
    Regrouped G;
    PhaseAPass(bool seed, bool main_, bool before) : do_seed(seed), do_main(main_), seeded_before(before), seeds_clean(!seed) {}
};

// Seed step: q-gram bounds of every pair of the pass and the pairs with the smallest bounds, or every entry against its 64 nearest longer
// neighbours, one wave per entry.
int phase_a_seeds(NNContext &C, const QMap &Q, PhaseAPass &P, HostClock &clk)
{
    int rc;
    if (P.bounds_wanted && !variant("nn_old_seed")) {
        if ((rc = C.build_bounds(Q, 63, P.PR, true))) return rc;
        P.bounds_built = true;
        clk.lap("phaseA: q-gram bounds");
        if (C.seeds_ready) {
            if ((rc = C.run_bound_seeds(Q))) return rc;
            P.bound_seeded = P.seeds_clean = true;
            clk.lap("phaseA: seed pairs");
            return ISOCON_OK;
        }
    }
    C.tm.start();
    hipLaunchKernelGGL(k_nn_scan_up<1>, dim3((Q.count() + 3) / 4), dim3(256), 0, 0, C.st->dev, C.params(63), Q, 0, 1, 1);
    ISO_HIP_CHECK(hipGetLastError());
    C.tm.stop_later(&C.stats.seed_kernel_ms);
    clk.lap("phaseA: seed kernel");
    return ISOCON_OK;
}

// Regrouping for the tile-synchronous kernels (whole-set calls the refill kernel cannot run -- it does not care how lanes are grouped):
// entries of EQUAL length are reordered by the connected component they fall into in the seed pass' "d <= 63" graph, so that the 64 lanes
// of a main-pass tile mostly hold sequences of one isoform and die (or survive) together.  Any order consistent with the lengths
// evaluates the same pair set; Regrouped::unpermute maps bounds and hits back.  A hit-list overflow leaves G empty: the end of the pass
// meets it again and restarts with a larger list.
int regroup_by_seed_hits(NNContext &C, const std::vector<int32_t> &best_at_entry, Regrouped &G, HostClock &clk)
{
    const uint32_t n = C.n;
    C.known_ready = false;          // (the seed pairs' table speaks of the caller's positions and of a hit list that is collected here)
    uint64_t needed0 = 0;
    std::vector<int32_t> seed_hits;
    int rc = C.collect(seed_hits, &needed0);
    if (rc == ISOCON_E_CAPACITY) return ISOCON_OK;
    if (rc || (rc = C.download_best())) return rc;
    G.seed_got.swap(seed_hits);
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t i = 0; i + 2 < G.seed_got.size(); i += 3) {
        if (G.seed_got[i + 2] < 0) continue;
        const uint32_t a = find((uint32_t)G.seed_got[i]), b = find((uint32_t)G.seed_got[i + 1]);
        if (a != b) parent[a < b ? b : a] = a < b ? a : b;
    }
    std::vector<uint32_t> &perm = G.perm;
    perm.resize(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::vector<uint32_t> root(n);
    for (uint32_t i = 0; i < n; ++i) root[i] = find(i);
    const std::vector<int32_t> &lens = C.st->lens;
    std::sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        if (lens[x] != lens[y]) return lens[x] < lens[y];
        if (root[x] != root[y]) return root[x] < root[y];
        if (C.best[x] != C.best[y]) return C.best[x] < C.best[y];   // proxy of the read's own error count
        return x < y;
    });
    if (clk.on) {
        std::vector<uint8_t> seen(n, 0);
        bool okp = true;
        for (uint32_t i = 0; i < n; ++i) { if (seen[perm[i]]) okp = false; seen[perm[i]] = 1; }
        size_t ncomp = 0, moved = 0;
        for (uint32_t i = 0; i < n; ++i) { ncomp += root[i] == i; moved += perm[i] != i; }
        bool lens_ok = true;
        for (uint32_t i = 0; i < n; ++i) lens_ok = lens_ok && lens[perm[i]] == lens[i];
        fprintf(stderr, "[isocon] regroup: n=%u components=%zu moved=%zu perm_valid=%d lens_preserved=%d seed_hits=%zu\n",
                n, ncomp, moved, (int)okp, (int)lens_ok, G.seed_got.size() / 3);
    }
    bool identity = true;
    for (uint32_t i = 0; i < n && identity; ++i) identity = perm[i] == i;
    if (identity) perm.clear();
    else {
        DevBuf d_planes2(&C.st->pool, SLOT_NN_PLANES2), d_perm(&C.st->pool, SLOT_NN_PERM);          // (pool slots: they outlive the handles)
        const size_t pbytes = (size_t)n * C.st->dev.nchunks * 16;
        if ((rc = d_planes2.alloc(pbytes)) || (rc = d_perm.alloc((size_t)n * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_perm.p, perm.data(), (size_t)n * 4));
        C.tm.start();
        hipLaunchKernelGGL(k_permute_planes, dim3(2048), dim3(256), 0, 0, reinterpret_cast<const ulonglong2 *>(C.st->dev.planes),
                           d_planes2.as<ulonglong2>(), d_perm.as<uint32_t>(), n, C.st->dev.nchunks);
        ISO_HIP_CHECK(hipGetLastError());
        C.tm.stop();
        G.planes = d_planes2.as<uint64_t>();
        G.best_at_entry = &best_at_entry;
        std::vector<int32_t> b2(n);
        std::vector<uint8_t> q2(n), t2(n);
        for (uint32_t i = 0; i < n; ++i) { b2[i] = C.best[perm[i]]; q2[i] = C.dev_excluded(perm[i]) ? 0 : C.qflag[perm[i]]; t2[i] = C.dev_excluded(perm[i]) ? 0 : C.tflag[perm[i]]; }
        ISO_HIP_CHECK(copy_h2d(C.d_best.p, b2.data(), (size_t)n * 4));
        ISO_HIP_CHECK(copy_h2d(C.d_qf.p, q2.data(), n));
        ISO_HIP_CHECK(copy_h2d(C.d_tf.p, t2.data(), n));
    }
    if ((rc = C.reset_counters())) return rc;
    G.seed_collected = true;
    clk.lap("phaseA: regroup (host+permute)");
    return ISOCON_OK;
}

// Listed main pass: the survivors of the bounds as the list builder and the block filter left them -- the 64-row tables, the 32-row
// tables, then the flat pairs (and the chunks too small for a table, converted to pairs) one per lane.
int run_listed_pass(NNContext &C, const QMap &Q, const NNParams &PR, const NNContext::ListPlan &LP)
{
    int rc;
    NNParams PL = PR;
    PL.list = C.d_list.as<uint32_t>();
    PL.slot_order = nullptr;
    // (the two launches side by side on two streams: no gain -- both are bound by VALU issue; profiles/r03c_sweep_side_stream_list_min.txt)
    // waves per table workgroup: 4 for the 64-row class (8.53 against 8.77 ms at C3 with 8: fewer lanes wait for a chunk's last pairs,
    // and residency is not what binds the launch -- DESIGN 4.4), 8 for the 32-row class (0.86 against 0.94 ms); nn_list_waves= overrides both
    const char *lw = variant_value("nn_list_waves");
    if ((LP.n_chunks || LP.n_chunks_narrow) && !C.build_text()) return ISOCON_E_HIP;
    if (LP.n_chunks) {
        // the 64-row class; largest chunks first (the sorted tables sit behind the unsorted ones)
        hipLaunchKernelGGL(k_nn_sort_chunks, dim3(1), dim3(1024), 0, 0, LP.a, (uint32_t)LP.n_chunks, LP.sorted_a);
        ISO_HIP_CHECK(hipGetLastError());
        PL.chunks = LP.sorted_a;
        const char *pad = variant_value("nn_lds_pad");
        const NNRefillShape sh = pad ? nn_refill_shape_padded(C.st->maxlen, atoi(pad)) : nn_refill_shape(C.st->maxlen, lw ? atoi(lw) : 4, false);
        if ((rc = launch_refill(C, sh, false, (unsigned)LP.n_chunks, PL, Q, 0))) return rc;
    }
    if (LP.n_chunks_narrow) {
        // the 32-row class (thresholds <= 31, nn_list.hpp): its own chunk table, its own counters, half the LDS per table
        C.tm.mark();
        hipLaunchKernelGGL(k_nn_sort_chunks, dim3(1), dim3(1024), 0, 0, LP.b, (uint32_t)LP.n_chunks_narrow, LP.sorted_b);
        ISO_HIP_CHECK(hipGetLastError());
        PL.chunks = LP.sorted_b;
        PL.stats = C.d_stats.as<unsigned long long>() + (NN_COUNTER_SLOTS * 4 + 1);
        if ((rc = launch_refill(C, nn_refill_shape(C.st->maxlen, lw ? atoi(lw) : 8, true), true, (unsigned)LP.n_chunks_narrow, PL, Q, 0))) return rc;
    }
    // The flat pairs: what the list builder and the filter left (LP.n_small, the pairs the seed pass has settled taken out already) and the
    // pairs of the converted chunks -- of those the host knows only the upper bound conv_pairs: k_nn_chunks_to_pairs takes the settled
    // ones out too, and the lane launch reads the number that is left on the device (no further wait of the host).
    const unsigned long long n_small = LP.n_small + LP.conv_pairs;
    const unsigned long long dropped = LP.K.drop ? LP.seed_known : 0;          // reached this stage and were not aligned a second time
    if (n_small) {
        C.tm.stop_later(&C.stats.scan_kernel_ms);
        C.tm.start();
        const unsigned long long pairs_cap = C.st->pool.slots[SLOT_NN_LPA].cap / 4;
        unsigned long long *known_count = C.d_stats.as<unsigned long long>() + NNContext::KNOWN_COUNTER;
        const unsigned long long *live = nullptr;
        if (LP.conv_a) hipLaunchKernelGGL(k_nn_chunks_to_pairs, dim3((unsigned)LP.conv_a), dim3(256), 0, 0, LP.a, C.d_list.as<uint32_t>(), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(), pairs_cap, C.d_ltot.as<NNPlanTotals>(), LP.K, known_count);
        if (LP.conv_b) hipLaunchKernelGGL(k_nn_chunks_to_pairs, dim3((unsigned)LP.conv_b), dim3(256), 0, 0, LP.b, C.d_list.as<uint32_t>(), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(), pairs_cap, C.d_ltot.as<NNPlanTotals>(), LP.K, known_count);
        if ((LP.conv_a || LP.conv_b) && LP.K.drop) live = &C.d_ltot.as<NNPlanTotals>()->n_small;
        hipLaunchKernelGGL(k_ed_lanes<true>, dim3((unsigned)((n_small + 255) / 256)), dim3(256), 0, 0, C.st->dev, C.params(63), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(),
                           (const int32_t *)nullptr, (uint64_t)n_small, (int32_t *)nullptr, live);
        ISO_HIP_CHECK(hipGetLastError());
        C.tm.stop_later(&C.stats.lanes_kernel_ms);
        C.tm.start();
    }
    // pairs_evaluated / pairs_lanes: the pairs that reached the alignment stage, settled ones included; pairs_lanes_aligned: what the launch
    // ran (the settled pairs of the converted chunks leave it when their counter arrives, NNContext::add_counters)
    C.stats.pairs_evaluated += n_small + dropped;
    C.stats.pairs_lanes += n_small + dropped;
    C.stats.pairs_seed_known += LP.seed_known;
    C.stats.pairs_lanes_aligned += n_small;
    return ISOCON_OK;
}

// Unlisted main pass, one workgroup per entry: the refill kernel by its own admission (roles, lengths, the bounds if PR has them), or -- the
// refill kernel is out -- the tile-synchronous kernels on interleaved planes (of the regrouped copy, if any).
int run_unlisted_pass(NNContext &C, const QMap &Q, const PhaseAPass &P, bool refill)
{
    const uint32_t nq = Q.count();
    // tile 0 = the pairs of the 64-neighbour seed pass (on a regrouped copy its "64 nearest" are other pairs: tile 0 again).  Seeds chosen
    // by their bounds are anywhere in the window, and a sharded call cannot know how the seeding call chose them: with the bounds in use
    // the pass starts at tile 0 (the few pairs met twice are dropped by isocon_nn_finalize).
    const int32_t first_tile = (P.G.perm.empty() && ((P.do_seed && !P.bound_seeded) || (P.seeded_before && !P.bounds_wanted))) ? 1 : 0;
    if (refill) {
        if (!C.build_text()) return ISOCON_E_HIP;
        // With the bounds in use a query keeps ~1/8 of its pairs: 512 lanes per table would get one or two pairs each and
        // wait for the slowest (72 % of the executed lane-columns live at C3); 256 lanes: 83 %, 54 -> 48 ms, although
        // only 12 waves per CU are left (3 workgroups by LDS).  variant nn_waves=8 / 4 overrides.
        const char *wv = variant_value("nn_waves");
        const bool four = wv ? atoi(wv) == 4 : P.PR.lb != nullptr;
        return launch_refill(C, nn_refill_shape(C.st->maxlen, four ? 4 : 8, false), false, nq, P.PR, Q, first_tile);
    }
    DevStore S = C.st->dev;
    if (P.G.planes) S.planes = P.G.planes;
    const NNTileScan kernel = nn_tile_scan(C.st->maxlen);
    const size_t lds = nn_tile_scan_lds(C.st->maxlen);
    if (kernel == NN_SCAN_WINDOW) {
        hipLaunchKernelGGL(k_nn_scan_up<1>, dim3(nq), dim3(256), 0, 0, S, C.params(63), Q, first_tile, 0x7fffffff, 4);
        return ISOCON_OK;
    }
    // lane texts with interleaved code bits
    DevBuf d_il(&C.st->pool, SLOT_NN_IL2);
    const size_t total = (size_t)C.n * C.st->dev.nchunks;
    int rc;
    if ((rc = d_il.alloc(total * 16))) return rc;
    hipLaunchKernelGGL(k_interleave_planes, dim3(2048), dim3(256), 0, 0, reinterpret_cast<const ulonglong2 *>(S.planes), d_il.as<ulonglong2>(), total);
    S.il = d_il.as<uint64_t>();
    if (kernel == NN_SCAN_LDS8) {
        hipLaunchKernelGGL(k_nn_scan_lds<8>, dim3(nq), dim3(512), lds, 0, S, C.params(63), Q, first_tile, 0x7fffffff);
    } else {
        ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_lds<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_nn_scan_lds<16>, dim3(nq), dim3(1024), lds, 0, S, C.params(63), Q, first_tile, 0x7fffffff);
    }
    return ISOCON_OK;
}

// Main pass: the rest of the window, thresholds tighten through best[].  With the refill kernel: bounds (unless the seed step built
// them), survivor lists, and the listed pass if the lists pay; otherwise one workgroup per entry.
int phase_a_main(NNContext &C, const QMap &Q, PhaseAPass &P, HostClock &clk)
{
    int rc;
    if (C.n >= (1u << 30)) { g_last_error = "store too large for the packed neighbour queue"; return ISOCON_E_ARG; }
    C.tm.start();
    // lane texts as nibbles, one fixed-stride row per sequence: room now, built in front of the first launch that reads them
    const bool refill = P.refill_main && P.G.perm.empty() && C.text_affordable();
    NNParams &PR = P.PR;
    if (refill && P.bounds_wanted && !P.bounds_built) {
        // q-gram bounds of every pair of the pass (outside the main kernel's own event pair: bound_kernel_ms)
        C.tm.stop_later(&C.stats.scan_kernel_ms);
        if ((rc = C.build_bounds(Q, 63, PR))) return rc;
        clk.lap("phaseA: q-gram bounds");
        C.tm.start();
    }
    if (!refill) { PR.lb = nullptr; PR.lb_row = nullptr; PR.slot_order = nullptr; }
    NNContext::ListPlan LP;
    if (refill && PR.lb != nullptr) {
        // the survivors of the bounds as lists, through the block filter: tables only for entries with enough pairs, and only their pairs
        C.tm.stop_later(&C.stats.scan_kernel_ms);
        if ((rc = C.plan_lists(Q, Q.count(), PR, LP))) return rc;
        clk.lap("phaseA: survivor lists");
        C.tm.start();
    }
    P.no_markers = LP.listed && P.seeds_clean;
    if ((rc = LP.listed ? run_listed_pass(C, Q, PR, LP) : run_unlisted_pass(C, Q, P, refill))) return rc;
    ISO_HIP_CHECK(hipGetLastError());
    C.tm.stop_later(&C.stats.scan_kernel_ms);
    C.stats.scan_launches += 1;
    return ISOCON_OK;
}

// 2-set, many candidates, no bounds (what nn_no_qgram leaves of the 2-set lists): the unlisted refill launch from tile 0 -- the same
// upward scan as the 1-set search; the role flags make a pair admissible only if one end is a read and the other a candidate; the pair
// belongs to its LOWER index, whatever its role.
int phase_a_two_set_unbounded(NNContext &C, const QMap &Q)
{
    C.tm.start();
    if (!C.build_text()) return ISOCON_E_HIP;
    int rc;
    if ((rc = launch_refill(C, nn_refill_shape(C.st->maxlen, 8, false), false, Q.count(), C.params(63), Q, 0))) return rc;
    C.tm.stop_later(&C.stats.scan_kernel_ms);
    C.stats.scan_launches += 1;
    return ISOCON_OK;
}

// 2-set, few candidates (or sequences too long for the LDS planes): explicit tiles -- shared = candidate, lanes = the shard's reads whose
// length is within 63 of the candidate's.
int phase_a_two_set_tiles(NNContext &C, const QMap &Q, bool do_main)
{
    std::vector<uint32_t> ts, ids, lanes;
    for (uint32_t c = 0; c < C.n && do_main; ++c) {
        if (!C.tflag[c] || C.dev_excluded(c)) continue;
        uint32_t lo, hi;
        length_window(C.st->lens, c, 63, lo, hi);
        lo = std::max(lo, Q.begin);
        hi = std::min(hi, Q.end);
        lanes.clear();
        for (uint32_t p = lo; p < hi; ++p)
            if (C.qflag[p] && !C.dev_excluded(p) && Q.owns(p)) lanes.push_back(p);
        push_tiles(ts, ids, c, lanes);
    }
    float ms = 0.f;
    int rc;
    if ((rc = run_nn_tiles(1, C, ts, ids, &ms))) return rc;
    C.stats.scan_launches += 1;
    C.stats.scan_kernel_ms += ms;
    return ISOCON_OK;
}

// End of a pass (the 64-row phase and the wide stages): the hits come to the host -- or stay on the device for the CSR kernels -- with
// the counters; an overflowed hit list is enlarged and `again` set (the caller runs the pass once more, bounds kept); the "-2" markers
// (a tile's window could not certify the pair) are resolved with cap `kcap` and applied.  G: the regrouped copy the pass ran on, if any.
int nn_end_pass(NNContext &C, int32_t kcap, bool no_markers, const Regrouped &G, HostClock *clk, bool &again)
{
    auto lap = [&](const char *what) { if (clk) clk->lap(what); };
    again = false;
    uint64_t needed = 0;
    std::vector<int32_t> got;
    const bool in_place = G.perm.empty();
    // single-GPU graph, ordinary case: the hits stay on the device for the CSR kernels (nn_finalize.hpp); nothing to post-process
    const bool dev_ok = C.keep_dev && no_markers && in_place && !G.seed_collected && C.hits.empty();
    const bool one_record = dev_ok && C.csr_follows && !C.st->n_exc && !C.flags_dirty;          // (the record reads the device's query flags: they must be the context's)
    int rc = one_record ? C.collect_record(&needed) : C.collect(got, &needed, in_place, dev_ok);    // (a regrouped run keeps best[] in permuted positions: no filter)
    C.tm.resolve();          // (behind the wait of the collect: the events are all reached)
    if (rc == ISOCON_E_CAPACITY) {   // the hit list overflowed: run again with a larger one
        C.hits_cap = needed + needed / 2 + 1024;
        if ((rc = C.d_hits.alloc(C.hits_cap * 12))) return rc;
        again = true;
        // Keep the bounds reached so far: every pair that attains a final bound is found again (d <= best holds
        // for it), the stale hits are not, and the second run is the cheap one (measured at 200 k reads: 2.6 s
        // instead of 5.4 s -- thresholds are final from the first pair on).
        if (in_place) return C.download_best();
        C.best = *G.best_at_entry;          // regrouped copy: bounds sit in permuted positions, simply start over
        return C.upload_flags();
    }
    if (rc) return rc;
    if (one_record) { lap("phaseA: hits and bounds stay on the device"); return ISOCON_OK; }
    if ((rc = C.download_best())) return rc;
    if (dev_ok) { lap("phaseA: hits stay on the device"); return ISOCON_OK; }
    if (!in_place && (rc = G.unpermute(C, got))) return rc;
    if (G.seed_collected) got.insert(got.end(), G.seed_got.begin(), G.seed_got.end());
    lap("phaseA: collect+unpermute");
    // split markers from real hits (the lane-refill kernels never emit markers)
    std::vector<uint32_t> ra, rb;
    for (size_t i = 0; i + 2 < got.size(); i += 3) {
        if (got[i + 2] == -2) { ra.push_back((uint32_t)got[i]); rb.push_back((uint32_t)got[i + 1]); }
        else C.hits.insert(C.hits.end(), got.begin() + i, got.begin() + i + 3);
    }
    if (!ra.empty()) {
        std::vector<int32_t> kk(ra.size(), kcap), dd(ra.size(), -1);
        float ems = 0.f;
        if ((rc = ed_pairs_impl(C.st, ra.data(), rb.data(), kk.data(), ra.size(), dd.data(), &ems, nullptr, C.image_pass))) return rc;
        C.tm.total += ems;
        for (size_t i = 0; i < ra.size(); ++i)
            if (dd[i] >= 0) C.apply(ra[i], rb[i], dd[i]);
    }
    lap("phaseA: markers");
    return ISOCON_OK;
}

// Phase A over the shard Q: the pairs of ordinary entries (bit-vector kernels).
int nn_phase_a_planes(NNContext &C, const QMap &Q, bool allow_regroup = false,
                      bool do_seed = true, bool do_main = true, bool seeded_before = false)
{
    const uint32_t n = C.n;
    if (Q.begin >= Q.end) return ISOCON_OK;
    const std::vector<int32_t> best0 = C.best;
    HostClock clk;
    const bool fits = nn_refill64_fits(C.st->maxlen);
    // reads vs MANY candidates (the statistical filter's reassignment rounds: thousands of near-identical candidates) go the way of
    // the 1-set search -- bounds, seeds from the smallest bounds, survivor lists owned by the hubs (here: the candidates): the role
    // flags make a pair admissible only between a read and a candidate.  Without the bounds (nn_no_qgram, a debug variant: nothing else
    // gets there) what is left of that is phase_a_two_set_unbounded.  Few candidates: explicit tiles (no bound matrix over read-read
    // pairs that can never be edges, and tiles are cheaper than a table per entry).
    const bool two_set_many = C.two_set && do_main && !variant("nn_tiles") && n < (1u << 30) && fits &&
                              (size_t)std::count(C.tflag.begin(), C.tflag.end(), (uint8_t)1) > 512;
    const bool two_set_lists = two_set_many && !variant("nn_no_qgram");
    const bool whole_set = Q.begin == 0 && Q.end == n && Q.stride == 1 && Q.block_log2 == 0 && C.depth >= n;
    for (;;) {
        int rc;
        if ((rc = C.begin_pass())) return rc;
        clk.lap("phaseA: upload/reset");
        PhaseAPass P(do_seed, do_main, seeded_before);
        if (!C.two_set || two_set_lists) {
            P.refill_main = !variant("nn_tiles") && fits;
            P.bounds_wanted = P.refill_main && !variant("nn_no_qgram");
            P.PR = C.params(63);
            if (do_seed && (rc = phase_a_seeds(C, Q, P, clk))) return rc;
            if (allow_regroup && !P.refill_main && do_seed && do_main && whole_set && n > 128 && (rc = regroup_by_seed_hits(C, best0, P.G, clk))) return rc;
            if (do_main && (rc = phase_a_main(C, Q, P, clk))) return rc;
            if (!do_main) P.no_markers = do_seed && P.seeds_clean;          // a seed-only phase: k_ed_lanes alone
            clk.lap("phaseA: main kernel");
        } else if (two_set_many && C.text_affordable()) {
            if ((rc = phase_a_two_set_unbounded(C, Q))) return rc;
        } else if ((rc = phase_a_two_set_tiles(C, Q, do_main))) return rc;
        bool again = false;
        if ((rc = nn_end_pass(C, 63, P.no_markers, P.G, &clk, again))) return rc;
        if (!again) return ISOCON_OK;
    }
}

}  // namespace
