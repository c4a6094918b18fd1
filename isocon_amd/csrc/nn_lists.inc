// nn_lists.inc -- NNContext::plan_lists: the survivors of the bounds as lists and chunk tables (nn_list.hpp) (included by isocon_hip.hip behind nn_context.inc).

namespace {

int NNContext::plan_lists(const QMap &Q, uint32_t nq, const NNParams &PR, ListPlan &L)
{
    L = ListPlan();
    if (PR.lb == nullptr || nq == 0 || variant("nn_no_list") || st->pool.slots[SLOT_NN_LBT].p == nullptr || st->maxlen >= 16384) return ISOCON_OK;
    unsigned long long pairs_cap = std::min<unsigned long long>(lb_total, std::max<unsigned long long>(1ull << 22, lb_total / 8));
    if (const char *e = variant_value("nn_list_cap")) pairs_cap = std::max<unsigned long long>(1, strtoull(e, nullptr, 10));      // tests: force the fallback
    // The block filter (nn_filter.hpp) sits between the list builder and the alignment launches: the builder then hands over the pairs of
    // every owner with at least NNF_LIST_MIN of them as chunks (the filter's cost per chunk is a 8 KB bitmap), and `list_min` decides what
    // the FILTER leaves as a chunk for the table kernels.  Without the filter the builder applies list_min itself.
    const bool filter = !variant("nn_no_block_filter") && ensure_text2();
    uint32_t list_min = NN_LIST_MIN;
    if (const char *e = variant_value("nn_list_min")) list_min = (uint32_t)std::max(1, atoi(e));        // A/B runs
    const uint32_t build_min = filter ? std::min<uint32_t>(list_min, NNF_LIST_MIN) : list_min;
    const unsigned long long cap_in = pairs_cap / build_min + 1, cap_out = filter ? pairs_cap / list_min + 1 : cap_in;
    size_t free_b = 0;
    if (!free_mem(free_b) || pairs_cap * 12 > free_b / 2 + st->pool.slots[SLOT_NN_LIST].cap * 3) return ISOCON_OK;
    DevBuf *bufs[] = {&d_ltot, &d_lchunks, &d_list, &d_lpa, &d_lpb, &d_lmeta, &d_ltasks};
    const int slots[] = {SLOT_NN_LTOT, SLOT_NN_LCHUNKS, SLOT_NN_LIST, SLOT_NN_LPA, SLOT_NN_LPB, SLOT_NN_LDEST, SLOT_NN_LTASKS};
    for (int i = 0; i < 7; ++i) { bufs[i]->pool = &st->pool; bufs[i]->slot = slots[i]; }
    // second pass of the filter: at most one task per chunk of the builder plus one per 64 surviving pairs
    const bool second = filter && !variant("nn_filter_one_pass");
    const unsigned long long tasks_cap = second ? 2 * cap_in + pairs_cap / 64 + 1 : 0;
    if (second && d_ltasks.alloc((size_t)tasks_cap * sizeof(NNFTask))) return ISOCON_OK;
    const size_t n_records = (size_t)(filter ? 2 * cap_in : 0) + 4 * (size_t)cap_out;
    if (d_lmeta.alloc(nn_meta_bytes(n)) || d_ltot.alloc(sizeof(NNPlanTotals)) || d_lchunks.alloc(n_records * sizeof(NNChunk)) || d_list.alloc((size_t)pairs_cap * 4) ||
        d_lpa.alloc((size_t)pairs_cap * 4) || d_lpb.alloc((size_t)pairs_cap * 4))
        return ISOCON_OK;
    // [builder: a, b (cap_in each; only with the filter)] [a, b as the alignment launches get them (cap_out each)] [their sorted copies]
    NNChunk *built = d_lchunks.as<NNChunk>();
    L.a = built + (filter ? 2 * cap_in : 0);
    L.b = L.a + cap_out;
    L.sorted_a = L.b + cap_out;
    L.sorted_b = L.sorted_a + cap_out;
    ISO_HIP_CHECK(hipMemsetAsync(d_ltot.p, 0, sizeof(NNPlanTotals), 0));
    NNBoundRows B;
    B.lb = PR.lb; B.row_off = PR.lb_row; B.row_len = lb_len_dev;
    B.lbT = static_cast<const uint8_t *>(st->pool.slots[SLOT_NN_LBT].p);
    B.offT = static_cast<const unsigned long long *>(st->pool.slots[SLOT_NN_LBT_OFF].p);
    B.sloT = static_cast<const uint32_t *>(st->pool.slots[SLOT_NN_LBT_SLO].p);
    B.lenT = static_cast<const uint32_t *>(st->pool.slots[SLOT_NN_LBT_LEN].p);
    B.score = static_cast<const uint32_t *>(st->pool.slots[SLOT_NN_SCORE].p);
    const NNSeedKnown K = seed_known();          // the pairs the seed pass of this pass has settled do not become flat pairs again
    tm.start();
    int32_t class_mode = 0;          // variant nn_narrow=0: every pair on 64 rows; =1: pairs above 31 leave the lists for the pair-per-lane kernel (nn_list.hpp)
    if (const char *e = variant_value("nn_narrow")) class_mode = atoi(e) > 0 ? 1 : -1;
    const NNSurvSide side = nn_surv_side(d_lmeta.as<uint32_t>(), n);          // the partners' items for the packed test, behind the meta words
    // four pairs per instruction, or pair by pair (variant nn_surv_scalar: A/B runs, tests)
    auto *const survivors = nn_surv_packed(PR.kcap, class_mode) && !variant("nn_surv_scalar") ? k_nn_survivors<true> : k_nn_survivors<false>;
    hipLaunchKernelGGL(k_nn_entry_meta, dim3((n + NN_META_PAD + 255) / 256), dim3(256), 0, 0, st->dev, PR, B.score, d_lmeta.as<uint32_t>(), side, d_ltot.as<NNPlanTotals>());
    ISO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(survivors, dim3((n + NN_SURV_WAVES - 1) / NN_SURV_WAVES), dim3(64 * NN_SURV_WAVES), 0, 0, st->dev, PR, B, d_lmeta.as<uint32_t>(), side, Q, nq, d_list.as<uint32_t>(), pairs_cap,
                       filter ? built : L.a, cap_in, d_lpa.as<uint32_t>(), d_lpb.as<uint32_t>(), pairs_cap, d_ltot.as<NNPlanTotals>(), build_min, class_mode, K);
    ISO_HIP_CHECK(hipGetLastError());
    if (filter) {
        // one launch over a work queue of the builder's chunks (their number is only known on the device)
        tm.mark();
        ISO_HIP_CHECK(nnf_launch_filter(d_text2.as<uint32_t>(), text2_stride, st->dev.lens, d_lmeta.as<uint32_t>(), PR.kcap, d_list.as<uint32_t>(), built, cap_in, L.a, cap_out,
                                        d_lpa.as<uint32_t>(), d_lpb.as<uint32_t>(), pairs_cap, d_ltot.as<NNPlanTotals>(), list_min,
                                        second ? d_ltasks.as<NNFTask>() : (NNFTask *)nullptr, tasks_cap, K));
    }
    tm.stop_later(&stats.list_kernel_ms, &stats.filter_kernel_ms);          // (the filter's part of list_kernel_ms; the context's own marked time is narrow_kernel_ms)
    // (the interval closes in front of the copy of the totals, not behind it as it used to: list_kernel_ms is the kernels' time alone)
    // the one answer the host cannot go on without: how many chunks and pairs the filter left decides which launches follow
    NNPlanTotals tot;
    ISO_HIP_CHECK(memcpy_wait(&tot, d_ltot.p, sizeof(tot), hipMemcpyDeviceToHost));
    if (tot.overflow) return ISOCON_OK;      // the bounds reject too little: lists would not fit
    stats.pairs_prefiltered += tot.n_filtered;
    stats.pairs_block_rejected += tot.f_rejected + tot.f_rejected2;
    L.listed = true;
    L.n_chunks = filter ? tot.f_chunks : tot.n_chunks;
    L.n_chunks_narrow = filter ? tot.f_chunks_narrow : tot.n_chunks_narrow;
    L.n_small = tot.n_small;
    L.seed_known = tot.n_seed_known;
    L.K = K;
    stats.pairs_wide_to_lanes += tot.n_wide_pairs;
    unsigned long long table_chunks = NNF_TABLE_CHUNKS;
    if (const char *e = variant_value("nn_table_chunks")) table_chunks = strtoull(e, nullptr, 10);          // A/B runs, tests (0: tables whatever is left)
    if (filter && L.n_chunks + L.n_chunks_narrow > 0 && L.n_chunks + L.n_chunks_narrow < table_chunks) {
        // too few chunks for a table launch to fill the chip: their pairs join the flat pairs (k_nn_chunks_to_pairs, launched by the caller in
        // front of the pair-per-lane kernel and inside its event pair)
        if (tot.n_small + tot.f_listed > pairs_cap) return ISOCON_OK;
        L.conv_a = L.n_chunks; L.conv_b = L.n_chunks_narrow; L.conv_pairs = tot.f_listed;
        L.n_chunks = L.n_chunks_narrow = 0;
        return ISOCON_OK;
    }
    stats.pairs_narrow += filter ? tot.f_narrow_listed : tot.n_narrow_listed;
    return ISOCON_OK;
}

}  // namespace
