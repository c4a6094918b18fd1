// nn_main.inc -- nn_phase_a_planes: the 64-row phase -- bounds, seeds, survivor lists, the table launches and the pair-per-lane launch (included by isocon_hip.hip behind nn_context.inc).

namespace {

// Phase A over the shard Q: the pairs of ordinary entries (bit-vector kernels).
int nn_phase_a_planes(NNContext &C, const QMap &Q, bool allow_regroup = false,
                      bool do_seed = true, bool do_main = true, bool seeded_before = false)
{
    const uint32_t n = C.n;
    const uint32_t q_begin = Q.begin, q_end = Q.end;
    if (q_begin >= q_end) return ISOCON_OK;
    const std::vector<int32_t> best0 = C.best;
    HostClock clk;
    for (;;) {
        int rc;
        if ((rc = C.upload_best()) || (rc = C.reset_counters())) return rc;
        clk.lap("phaseA: upload/reset");
        float ms = 0.f;
        std::vector<uint32_t> perm_used;     // non-empty: the main pass ran on a regrouped copy of the store
        std::vector<int32_t> seed_got;       // seed-pass hits collected early (caller's positions)
        bool seed_collected = false;
        bool no_markers = false;             // the pass ran only kernels that never emit "re-run" markers (survivor lists, bound seeds)
        bool seeds_clean = !do_seed;         // (a sharded call runs the seeds and the lists in separate phases: each is judged by what IT launched)
        // reads vs MANY candidates (the statistical filter's reassignment rounds: thousands of near-identical candidates) go the way of
        // the 1-set search -- bounds, seeds from the smallest bounds, survivor lists owned by the hubs (here: the candidates): the role
        // flags make a pair admissible only between a read and a candidate.  Few candidates: explicit tiles below (no bound matrix over
        // read-read pairs that can never be edges).
        const bool two_set_lists = C.two_set && do_main && !variant("nn_tiles") && !variant("nn_no_qgram") &&
                                   n < (1u << 30) &&
                                   (size_t)std::count(C.tflag.begin(), C.tflag.end(), (uint8_t)1) > 512 &&
                                   ((size_t)4 * ((C.st->maxlen + 192 + 31) & ~31) + 160) * 4 + 16 * NN_RING * 8 + 16 <= (size_t)160 * 1024;
        if (!C.two_set || two_set_lists) {
            const uint32_t nq = Q.count();   // owned entries (launch slots)
            // seed pass: every entry against its 64 nearest longer neighbours, one wave per entry
            // (the lane-refill main pass does not care how lanes are grouped: no regrouping there)
            const bool refill_main = !variant("nn_tiles") &&
                                     ((size_t)4 * ((C.st->maxlen + 192 + 31) & ~31) + 160) * 4 + 16 * NN_RING * 8 + 16 <= (size_t)160 * 1024;
            const bool bounds_wanted = refill_main && !variant("nn_no_qgram");
            NNParams PR = C.params(63);
            bool bound_seeded = false, bounds_built = false;
            if (do_seed) {
                if (bounds_wanted && !variant("nn_old_seed")) {
                    // q-gram bounds of every pair of the pass first; the pairs with the smallest bounds are the seeds
                    if ((rc = C.build_bounds(Q, 63, PR, true))) return rc;
                    bounds_built = true;
                    clk.lap("phaseA: q-gram bounds");
                    if (C.seeds_ready) {
                        if ((rc = C.run_bound_seeds(Q))) return rc;
                        bound_seeded = true;
                        seeds_clean = true;
                        clk.lap("phaseA: seed pairs");
                    }
                }
                if (!bound_seeded) {
                    C.tm.start();
                    hipLaunchKernelGGL(k_nn_scan_up<1>, dim3((nq + 3) / 4), dim3(256), 0, 0, C.st->dev, C.params(63), Q, 0, 1, 1);
                    ISO_HIP_CHECK(hipGetLastError());
                    C.tm.stop_later(&C.stats.seed_kernel_ms);
                    clk.lap("phaseA: seed kernel");
                }
            }
            // Optional regrouping (whole-set calls only): entries of EQUAL length are reordered by the connected
            // component they fall into in the seed pass' "d <= 63" graph, so that the 64 lanes of a main-pass tile
            // mostly hold sequences of one isoform and die (or survive) together.  Any order consistent with the
            // lengths evaluates the same pair set; hits are mapped back to the caller's positions.
            std::vector<uint32_t> perm;
            DevStore S = C.st->dev;
            DevBuf d_planes2(&C.st->pool, SLOT_NN_PLANES2), d_perm(&C.st->pool, SLOT_NN_PERM), d_il(&C.st->pool, SLOT_NN_IL2);
            if (allow_regroup && !refill_main && do_seed && do_main && q_begin == 0 && q_end == n && Q.stride == 1 && Q.block_log2 == 0 && C.depth >= n && n > 128) {
                uint64_t needed0 = 0;
                std::vector<int32_t> seed_hits;
                rc = C.collect(seed_hits, &needed0);
                if (rc == ISOCON_OK) {
                    if ((rc = C.download_best())) return rc;
                    seed_got.swap(seed_hits);
                    std::vector<uint32_t> parent(n);
                    std::iota(parent.begin(), parent.end(), 0u);
                    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
                    for (size_t i = 0; i + 2 < seed_got.size(); i += 3) {
                        if (seed_got[i + 2] < 0) continue;
                        const uint32_t a = find((uint32_t)seed_got[i]), b = find((uint32_t)seed_got[i + 1]);
                        if (a != b) parent[a < b ? b : a] = a < b ? a : b;
                    }
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
                    if (getenv("ISOCON_DEBUG")) {
                        std::vector<uint8_t> seen(n, 0);
                        bool okp = true;
                        for (uint32_t i = 0; i < n; ++i) { if (seen[perm[i]]) okp = false; seen[perm[i]] = 1; }
                        size_t ncomp = 0, moved = 0;
                        for (uint32_t i = 0; i < n; ++i) { ncomp += root[i] == i; moved += perm[i] != i; }
                        bool lens_ok = true;
                        for (uint32_t i = 0; i < n; ++i) lens_ok = lens_ok && lens[perm[i]] == lens[i];
                        fprintf(stderr, "[isocon] regroup: n=%u components=%zu moved=%zu perm_valid=%d lens_preserved=%d seed_hits=%zu\n",
                                n, ncomp, moved, (int)okp, (int)lens_ok, seed_got.size() / 3);
                    }
                    bool identity = true;
                    for (uint32_t i = 0; i < n && identity; ++i) identity = perm[i] == i;
                    if (identity) perm.clear();
                    else {
                        const size_t pbytes = (size_t)n * C.st->dev.nchunks * 16;
                        if ((rc = d_planes2.alloc(pbytes)) || (rc = d_perm.alloc((size_t)n * 4))) return rc;
                        ISO_HIP_CHECK(copy_h2d(d_perm.p, perm.data(), (size_t)n * 4));
                        C.tm.start();
                        hipLaunchKernelGGL(k_permute_planes, dim3(2048), dim3(256), 0, 0, reinterpret_cast<const ulonglong2 *>(C.st->dev.planes),
                                           d_planes2.as<ulonglong2>(), d_perm.as<uint32_t>(), n, C.st->dev.nchunks);
                        ISO_HIP_CHECK(hipGetLastError());
                        C.tm.stop();
                        S.planes = d_planes2.as<uint64_t>();
                        std::vector<int32_t> b2(n);
                        std::vector<uint8_t> q2(n), t2(n);
                        for (uint32_t i = 0; i < n; ++i) { b2[i] = C.best[perm[i]]; q2[i] = C.dev_excluded(perm[i]) ? 0 : C.qflag[perm[i]]; t2[i] = C.dev_excluded(perm[i]) ? 0 : C.tflag[perm[i]]; }
                        ISO_HIP_CHECK(copy_h2d(C.d_best.p, b2.data(), (size_t)n * 4));
                        ISO_HIP_CHECK(copy_h2d(C.d_qf.p, q2.data(), n));
                        ISO_HIP_CHECK(copy_h2d(C.d_tf.p, t2.data(), n));
                    }
                    if ((rc = C.reset_counters())) return rc;
                    seed_collected = true;
                    clk.lap("phaseA: regroup (host+permute)");
                } else if (rc != ISOCON_E_CAPACITY) return rc;
                // on a hit-list overflow fall through: the common collect below restarts with a larger list
            }
            // main pass: the rest of the window, one workgroup per entry with the entry's window table in LDS,
            // thresholds tighten through best[]
            if (do_main) {
                const size_t lds = (size_t)(C.st->maxlen + 192) * 16;
                // on a regrouped copy the seed pass' "64 nearest" are other pairs: start from the first tile again
                // tile 0 = the pairs of the 64-neighbour seed pass.  Seeds chosen by their bounds are anywhere in the window, and
                // a sharded call cannot know how the seeding call chose them: with the bounds in use the pass starts at tile 0
                // (the few pairs met twice are dropped by isocon_nn_finalize).
                const int32_t first_tile = (perm.empty() && ((do_seed && !bound_seeded) || (seeded_before && !bounds_wanted))) ? 1 : 0;
                C.tm.start();
                const bool tiles_kernel = variant("nn_tiles");     // the tile-synchronous main pass (kept for A/B runs)
                const size_t lds_r = ((size_t)4 * ((C.st->maxlen + 192 + 31) & ~31) + 160) * 4;      // refill kernel: planes + virtual plane
                const size_t ring8 = 8 * NN_RING * 8 + 16, ring16 = 16 * NN_RING * 8 + 16, cu_lds = 160 * 1024;
                if (n >= (1u << 30)) { g_last_error = "store too large for the packed neighbour queue"; return ISOCON_E_ARG; }
                bool refill = !tiles_kernel && lds_r + ring16 <= cu_lds && perm.empty();
                if (refill) refill = C.text_affordable();          // lane texts as nibbles, one fixed-stride row per sequence: room now, built in front of the first launch that reads them
                const uint32_t text_stride = C.text_stride;
                DevBuf &d_il_text = C.d_text;
                if (!refill && lds <= 160 * 1024) {  // lane texts with interleaved code bits (of the regrouped copy, if any)
                    const size_t total = (size_t)n * C.st->dev.nchunks;
                    if ((rc = d_il.alloc(total * 16))) return rc;
                    hipLaunchKernelGGL(k_interleave_planes, dim3(2048), dim3(256), 0, 0, reinterpret_cast<const ulonglong2 *>(S.planes), d_il.as<ulonglong2>(), total);
                    S.il = d_il.as<uint64_t>();
                }
                if (refill && bounds_wanted && !bounds_built) {
                    // q-gram bounds of every pair of the pass (outside the main kernel's own event pair: bound_kernel_ms)
                    C.tm.stop_later(&C.stats.scan_kernel_ms);
                    if ((rc = C.build_bounds(Q, 63, PR))) return rc;
                    clk.lap("phaseA: q-gram bounds");
                    C.tm.start();
                }
                if (!refill) { PR.lb = nullptr; PR.lb_row = nullptr; PR.slot_order = nullptr; }
                // With the bounds in use a query keeps ~1/8 of its pairs: 512 lanes per table would get one or two pairs each and
                // wait for the slowest (72 % of the executed lane-columns live at C3); 256 lanes: 83 %, 54 -> 48 ms, although
                // only 12 waves per CU are left (3 workgroups by LDS).  variant nn_waves=8 / 4 overrides.
                const char *wv = variant_value("nn_waves");
                const bool four = wv ? atoi(wv) == 4 : PR.lb != nullptr;
                NNContext::ListPlan LP;
                if (refill && PR.lb != nullptr) {
                    // the survivors of the bounds as lists, through the block filter: tables only for entries with enough pairs, and only their pairs
                    C.tm.stop_later(&C.stats.scan_kernel_ms);
                    if ((rc = C.plan_lists(Q, nq, PR, LP))) return rc;
                    clk.lap("phaseA: survivor lists");
                    C.tm.start();
                }
                const bool listed = LP.listed;
                if (refill && !listed && !C.build_text()) return ISOCON_E_HIP;          // every launch of the chain below reads the text
                const unsigned long long n_chunks = LP.n_chunks, n_chunks_narrow = LP.n_chunks_narrow, n_small = LP.n_small + LP.conv_pairs;
                no_markers = listed && seeds_clean;
                if (listed) {
                    NNParams PL = PR;
                    PL.list = C.d_list.as<uint32_t>();
                    PL.slot_order = nullptr;
                    // (the two launches side by side on two streams: no gain -- both are bound by VALU issue; profiles/r03c_sweep_side_stream_list_min.txt)
                    // waves per table workgroup: 4 for the 64-row class (8.53 against 8.77 ms at C3 with 8: fewer lanes wait for a chunk's last pairs,
                    // and residency is not what binds the launch -- DESIGN 4.4), 8 for the 32-row class (0.86 against 0.94 ms); nn_list_waves= overrides both
                    const char *lw = variant_value("nn_list_waves");
                    const int lw64 = lw ? atoi(lw) : 4, lw32 = lw ? atoi(lw) : 8;
                    if ((n_chunks || n_chunks_narrow) && !C.build_text()) return ISOCON_E_HIP;
                    if (n_chunks) {
                        // the 64-row class; largest chunks first (the sorted tables sit behind the unsorted ones)
                        NNChunk *sorted = LP.sorted_a;
                        hipLaunchKernelGGL(k_nn_sort_chunks, dim3(1), dim3(1024), 0, 0, LP.a, (uint32_t)n_chunks, sorted);
                        ISO_HIP_CHECK(hipGetLastError());
                        PL.chunks = sorted;
                        if (const char *pad = variant_value("nn_lds_pad")) {
                            // occupancy experiment: the same launch with `pad` more bytes of LDS per workgroup (3 -> 2 -> 1 workgroups per CU)
                            const size_t lds_p = lds_r + (size_t)atoi(pad);
                            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<8, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p));
                            hipLaunchKernelGGL((k_nn_scan_refill<8, 1>), dim3((unsigned)n_chunks), dim3(512), lds_p, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        } else if (lw64 == 4 && 3 * (lds_r + ring8) <= cu_lds) {
                            hipLaunchKernelGGL((k_nn_scan_refill<4, 1>), dim3((unsigned)n_chunks), dim3(256), lds_r, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        } else if (3 * (lds_r + ring8) <= cu_lds) {
                            hipLaunchKernelGGL((k_nn_scan_refill<8, 1>), dim3((unsigned)n_chunks), dim3(512), lds_r, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        } else {
                            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<16, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r));
                            hipLaunchKernelGGL((k_nn_scan_refill<16, 1>), dim3((unsigned)n_chunks), dim3(1024), lds_r, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        }
                        ISO_HIP_CHECK(hipGetLastError());
                    }
                    if (n_chunks_narrow) {
                        // the 32-row class (thresholds <= 31, nn_list.hpp): its own chunk table, its own counters, half the LDS per table
                        C.tm.mark();
                        NNChunk *sorted = LP.sorted_b;
                        hipLaunchKernelGGL(k_nn_sort_chunks, dim3(1), dim3(1024), 0, 0, LP.b, (uint32_t)n_chunks_narrow, sorted);
                        ISO_HIP_CHECK(hipGetLastError());
                        PL.chunks = sorted;
                        PL.stats = C.d_stats.as<unsigned long long>() + (NN_COUNTER_SLOTS * 4 + 1);
                        const size_t lds_h = ((size_t)4 * ((C.st->maxlen + 96 + 31) & ~31) + 96) * 4;      // 32-row form: planes + virtual plane
                        if (lw32 == 4 && 3 * (lds_h + ring8) <= cu_lds) {
                            hipLaunchKernelGGL((k_nn_scan_refill<4, 1, true>), dim3((unsigned)n_chunks_narrow), dim3(256), lds_h, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        } else if (3 * (lds_h + ring8) <= cu_lds) {
                            hipLaunchKernelGGL((k_nn_scan_refill<8, 1, true>), dim3((unsigned)n_chunks_narrow), dim3(512), lds_h, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        } else {
                            ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<16, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_h));
                            hipLaunchKernelGGL((k_nn_scan_refill<16, 1, true>), dim3((unsigned)n_chunks_narrow), dim3(1024), lds_h, 0, S, PL, d_il_text.as<uint32_t>(), text_stride, Q, 0);
                        }
                        ISO_HIP_CHECK(hipGetLastError());
                        PL.stats = C.d_stats.as<unsigned long long>();
                    }
                    if (n_small) {
                        C.tm.stop_later(&C.stats.scan_kernel_ms);
                        C.tm.start();
                        const unsigned long long pairs_cap = C.st->pool.slots[SLOT_NN_LPA].cap / 4;
                        if (LP.conv_a) hipLaunchKernelGGL(k_nn_chunks_to_pairs, dim3((unsigned)LP.conv_a), dim3(256), 0, 0, LP.a, C.d_list.as<uint32_t>(), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(), pairs_cap, C.d_ltot.as<NNPlanTotals>());
                        if (LP.conv_b) hipLaunchKernelGGL(k_nn_chunks_to_pairs, dim3((unsigned)LP.conv_b), dim3(256), 0, 0, LP.b, C.d_list.as<uint32_t>(), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(), pairs_cap, C.d_ltot.as<NNPlanTotals>());
                        hipLaunchKernelGGL(k_ed_lanes<true>, dim3((unsigned)((n_small + 255) / 256)), dim3(256), 0, 0, C.st->dev, C.params(63), C.d_lpa.as<uint32_t>(), C.d_lpb.as<uint32_t>(),
                                           (const int32_t *)nullptr, (uint64_t)n_small, (int32_t *)nullptr);
                        ISO_HIP_CHECK(hipGetLastError());
                        C.tm.stop_later(&C.stats.lanes_kernel_ms);
                        C.stats.pairs_evaluated += n_small;
                        C.stats.pairs_lanes += n_small;
                        C.tm.start();
                    }
                } else if (refill && four && 3 * (lds_r + ring8) <= cu_lds) {
                    hipLaunchKernelGGL((k_nn_scan_refill<4, 1>), dim3(nq), dim3(256), lds_r, 0, S, PR, d_il_text.as<uint32_t>(), text_stride, Q, first_tile);
                } else if (refill && 3 * (lds_r + ring8) <= cu_lds) {
                    hipLaunchKernelGGL((k_nn_scan_refill<8, 1>), dim3(nq), dim3(512), lds_r, 0, S, PR, d_il_text.as<uint32_t>(), text_stride, Q, first_tile);
                } else if (refill) {
                    ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<16, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r));
                    hipLaunchKernelGGL((k_nn_scan_refill<16, 1>), dim3(nq), dim3(1024), lds_r, 0, S, PR, d_il_text.as<uint32_t>(), text_stride, Q, first_tile);
                } else if (lds <= 53 * 1024) {          // three 8-wave workgroups per CU
                    hipLaunchKernelGGL(k_nn_scan_lds<8>, dim3(nq), dim3(512), lds, 0, S, C.params(63), Q, first_tile, 0x7fffffff);
                } else if (lds <= 160 * 1024) {  // long reads: one 16-wave workgroup per table
                    ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_lds<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                    hipLaunchKernelGGL(k_nn_scan_lds<16>, dim3(nq), dim3(1024), lds, 0, S, C.params(63), Q, first_tile, 0x7fffffff);
                } else {                         // > 10 kb: scalar-window kernel
                    hipLaunchKernelGGL(k_nn_scan_up<1>, dim3(nq), dim3(256), 0, 0, S, C.params(63), Q, first_tile, 0x7fffffff, 4);
                }
                ISO_HIP_CHECK(hipGetLastError());
                C.tm.stop_later(&C.stats.scan_kernel_ms);
                C.stats.scan_launches += 1;
            }
            if (!do_main) no_markers = do_seed && seeds_clean;          // a seed-only phase: k_ed_lanes alone
            perm_used.swap(perm);
            clk.lap("phaseA: main kernel");
        } else if (do_main && !variant("nn_tiles") && n < (1u << 30) &&
                   (size_t)std::count(C.tflag.begin(), C.tflag.end(), (uint8_t)1) > 512 &&      // few candidates: explicit tiles are cheaper than a table per entry
                   ((size_t)4 * ((C.st->maxlen + 192 + 31) & ~31) + 160) * 4 + 16 * NN_RING * 8 + 16 <= (size_t)160 * 1024 && C.text_affordable()) {
            // reads vs candidates with the same upward scan as the 1-set search: the role flags make a pair admissible
            // only if one end is a read and the other a candidate; the pair belongs to its LOWER index, whatever its role
            const uint32_t nq = Q.count();
            const size_t lds_r = ((size_t)4 * ((C.st->maxlen + 192 + 31) & ~31) + 160) * 4, ring8 = 8 * NN_RING * 8 + 16;
            NNParams PR = C.params(63);
            if ((rc = C.build_bounds(Q, 63, PR))) return rc;
            C.tm.start();
            if (!C.build_text()) return ISOCON_E_HIP;
            if (3 * (lds_r + ring8) <= (size_t)160 * 1024) {
                hipLaunchKernelGGL((k_nn_scan_refill<8, 1>), dim3(nq), dim3(512), lds_r, 0, C.st->dev, PR, C.d_text.as<uint32_t>(), C.text_stride,
                                   Q, 0);
            } else {
                ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_nn_scan_refill<16, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r));
                hipLaunchKernelGGL((k_nn_scan_refill<16, 1>), dim3(nq), dim3(1024), lds_r, 0, C.st->dev, PR, C.d_text.as<uint32_t>(), C.text_stride,
                                   Q, 0);
            }
            ISO_HIP_CHECK(hipGetLastError());
            C.tm.stop_later(&C.stats.scan_kernel_ms);
            C.stats.scan_launches += 1;
        } else {
            // (fallback: sequences too long for the LDS planes)  shared = candidate, lanes = the shard's reads whose
            // length is within 63 of the candidate's
            std::vector<uint32_t> ts, ids, lanes;
            for (uint32_t c = 0; c < n && do_main; ++c) {
                if (!C.tflag[c] || C.dev_excluded(c)) continue;
                uint32_t lo, hi;
                length_window(C.st->lens, c, 63, lo, hi);
                lo = std::max(lo, q_begin);
                hi = std::min(hi, q_end);
                lanes.clear();
                for (uint32_t p = lo; p < hi; ++p)
                    if (C.qflag[p] && !C.dev_excluded(p) && Q.owns(p)) lanes.push_back(p);
                push_tiles(ts, ids, c, lanes);
            }
            if ((rc = run_nn_tiles(1, C, ts, ids, &ms))) return rc;
            C.stats.scan_launches += 1;
        }
        C.stats.scan_kernel_ms += ms;
        uint64_t needed = 0;
        std::vector<int32_t> got;
        // single-GPU graph, ordinary case: the hits stay on the device for the CSR kernels (nn_finalize.hpp); nothing to post-process
        const bool dev_ok = C.keep_dev && no_markers && perm_used.empty() && !seed_collected && C.hits.empty();
        const bool one_record = dev_ok && C.csr_follows && !C.st->n_exc && !C.flags_dirty;          // (the record reads the device's query flags: they must be the context's)
        rc = one_record ? C.collect_record(&needed) : C.collect(got, &needed, perm_used.empty(), dev_ok);    // (a regrouped run keeps best[] in permuted positions: no filter)
        C.tm.resolve();          // (behind the wait of the collect: the events are all reached)
        if (rc == ISOCON_E_CAPACITY) {   // the hit list overflowed: run again with a larger one
            C.hits_cap = needed + needed / 2 + 1024;
            if ((rc = C.d_hits.alloc(C.hits_cap * 12))) return rc;
            if (perm_used.empty()) {
                // Keep the bounds reached so far: every pair that attains a final bound is found again (d <= best holds
                // for it), the stale hits are not, and the second run is the cheap one (measured at 200 k reads: 2.6 s
                // instead of 5.4 s -- thresholds are final from the first pair on).
                if ((rc = C.download_best())) return rc;
            } else {                    // regrouped copy: bounds sit in permuted positions, simply start over
                C.best = best0;
                if ((rc = C.upload_flags())) return rc;
            }
            continue;
        }
        if (rc) return rc;
        if (one_record) { clk.lap("phaseA: hits and bounds stay on the device"); return ISOCON_OK; }
        if ((rc = C.download_best())) return rc;
        if (dev_ok) { clk.lap("phaseA: hits stay on the device"); return ISOCON_OK; }
        if (!perm_used.empty()) {           // back to the caller's positions
            std::vector<int32_t> b(n);
            for (uint32_t i = 0; i < n; ++i) b[perm_used[i]] = C.best[i];
            std::copy(b.begin(), b.end(), C.best.begin());
            for (size_t i = 0; i + 2 < got.size(); i += 3) { got[i] = (int32_t)perm_used[got[i]]; got[i + 1] = (int32_t)perm_used[got[i + 1]]; }
            if ((rc = C.upload_flags())) return rc;
        }
        if (seed_collected) got.insert(got.end(), seed_got.begin(), seed_got.end());
        clk.lap("phaseA: collect+unpermute");
        // split markers (-2: the tile's window could not certify the pair) from real hits
        std::vector<uint32_t> ra, rb;
        bool any_marker = false;
        for (size_t i = 2; i < got.size() && !any_marker; i += 3) any_marker = got[i] == -2;
        if (!any_marker) C.hits.insert(C.hits.end(), got.begin(), got.end());          // (the lane-refill kernels never emit markers)
        else {
            C.hits.reserve(C.hits.size() + got.size());
            for (size_t i = 0; i + 2 < got.size(); i += 3) {
                if (got[i + 2] == -2) { ra.push_back((uint32_t)got[i]); rb.push_back((uint32_t)got[i + 1]); }
                else C.hits.insert(C.hits.end(), got.begin() + i, got.begin() + i + 3);
            }
        }
        if (!ra.empty()) {
            std::vector<int32_t> kk(ra.size(), 63), dd(ra.size(), -1);
            float ems = 0.f;
            if ((rc = ed_pairs_impl(C.st, ra.data(), rb.data(), kk.data(), ra.size(), dd.data(), &ems, nullptr, C.image_pass))) return rc;
            C.tm.total += ems;
            for (size_t i = 0; i < ra.size(); ++i)
                if (dd[i] >= 0) C.apply(ra[i], rb[i], dd[i]);
        }
        clk.lap("phaseA: markers");
        return ISOCON_OK;
    }
}

// q_list != nullptr: the "sparse" launch of k_nn_scan_refill (nn.hpp) -- one workgroup per listed query instead of one per
// entry; pays when few entries act as queries (a workgroup per entry would run with one or two live lanes).

}  // namespace
