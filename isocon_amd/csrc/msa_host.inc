// msa_host.inc -- host side of the consensus correction (msa.hpp; included by isocon_hip.hip): one build of the matrices from CIGAR ops and
// one correction of built matrices, both on a batch of partitions; the single-partition entry points call them with a batch of one.

namespace {

template <class T> T *msa_slot(ScratchPool *pl, int slot) { return static_cast<T *>(pl->slots[slot].p); }

int msa_upload(ScratchPool *pl, int slot, const void *src, size_t bytes)
{
    DevBuf d(pl, slot);
    if (int rc = d.alloc(bytes)) return rc;
    if (bytes) ISO_HIP_CHECK(copy_h2d(d.p, src, bytes));
    return ISOCON_OK;
}

MsaBatch msa_batch_desc(ScratchPool *pl, uint32_t n_parts, uint32_t n_rows)
{
    MsaBatch B;
    B.part_of_row = msa_slot<const uint32_t>(pl, SLOT_MSA_PART);
    B.first_row = msa_slot<const uint32_t>(pl, SLOT_MSA_FIRST);
    B.Lm = msa_slot<const uint32_t>(pl, SLOT_MSA_LM);
    B.slot_base = msa_slot<const uint32_t>(pl, SLOT_MSA_SBASE);
    B.ncols = msa_slot<const uint32_t>(pl, SLOT_MSA_NCOLS);
    B.m_off = msa_slot<const unsigned long long>(pl, SLOT_MSA_MOFF);
    B.col_base = msa_slot<const uint32_t>(pl, SLOT_MSA_CBASE);
    B.n_parts = n_parts;
    B.n_rows = n_rows;
    return B;
}

// what a placed build hands back: the records of the slots it left to the host, and how many it placed
struct MsaPlaced {
    uint32_t *out_left;
    uint64_t left_cap, *n_left, *n_placed;
};

// The matrices of n_parts partitions from the ops of their rows (the arguments of isocon_msa_build_ops_batch), left in SLOT_MSA_IN and
// described by the store's pool->msa, tagged `by`.  A refused build leaves no build.
// placed != nullptr (isocon_msa_build_ops_placed[_batch]): the record list stays on the device -- sized here from the code-3 ops, an upper
// bound, so it never overflows; out_wide / wide_cap / n_wide are not used -- and the insertions of the wide slots are placed there
// (k_msa_slot_rep, k_msa_place); only the records of slots beyond PLACE_MAX_LONGEST come back.  Between fill and place the host waits for
// nothing: the number of wide slots comes with the one read after the layout, the record counts with the one read at the end.
int msa_build(isocon_store *s, MsaBuilt::By by, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
              uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide, uint64_t wide_cap, uint64_t *n_wide, float *kernel_ms,
              const MsaPlaced *placed = nullptr)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!s->acgt) { g_last_error = "the consensus correction needs a store over the alphabet ACGT"; return ISOCON_E_ALPHABET; }
    const char *centre_with_ops = by == MsaBuilt::SINGLE ? "row 0 is the centre: it has no ops" : "the first row of a partition is its centre: it has no ops";
    const uint32_t n = s->dev.n, n_rows = first_row[n_parts];
    if (first_row[0] != 0 || n_rows == 0) return ISOCON_E_ARG;
    std::vector<uint32_t> part_of_row(n_rows), Lm(n_parts), slot_base((size_t)n_parts + 1, 0);
    for (uint32_t p = 0; p < n_parts; ++p) {
        if (first_row[p + 1] <= first_row[p]) { g_last_error = "a partition without rows"; return ISOCON_E_ARG; }
        if (first_row[p + 1] > n_rows) { g_last_error = "a partition ends behind the last row"; return ISOCON_E_ARG; }          // (part_of_row has n_rows entries)
        for (uint32_t r = first_row[p]; r < first_row[p + 1]; ++r) {
            if (row_ids[r] >= n) { g_last_error = "row id out of range"; return ISOCON_E_ARG; }
            if (ops_ptr[r + 1] < ops_ptr[r]) return ISOCON_E_ARG;
            part_of_row[r] = p;
        }
        if (ops_ptr[first_row[p] + 1] != ops_ptr[first_row[p]]) { g_last_error = centre_with_ops; return ISOCON_E_ARG; }
        Lm[p] = (uint32_t)s->lens[row_ids[first_row[p]]];
        if ((uint64_t)slot_base[p] + Lm[p] + 1 > 0xffffffffull) { g_last_error = "too many insertion slots in one batch"; return ISOCON_E_UNSUPPORTED; }
        slot_base[p + 1] = slot_base[p] + Lm[p] + 1;
    }
    const uint64_t n_ops = ops_ptr[n_rows];
    if (ops_ptr[0] != 0) { g_last_error = centre_with_ops; return ISOCON_E_ARG; }
    if (n_ops && !ops) return ISOCON_E_ARG;
    const uint32_t n_slots = slot_base[n_parts];
    if (placed) {
        wide_cap = 0;
        for (uint64_t k = 0; k < n_ops; ++k) wide_cap += (ops[k] & 15u) == 3u;
    }
    ScratchPool *pl = &s->pool;
    MsaBuilt &H = pl->msa;
    H = MsaBuilt();
    DevBuf d_longest(pl, SLOT_MSA_LONGEST), d_width(pl, SLOT_MSA_WIDTH), d_cslot(pl, SLOT_MSA_CSLOT), d_tot(pl, SLOT_MSA_LTOT), d_wide(pl, SLOT_MSA_WIDE), d_M(pl, SLOT_MSA_IN),
        d_ncols(pl, SLOT_MSA_NCOLS), d_widx(pl, SLOT_MSA_WIDX), d_keys(pl, SLOT_MSA_KEYS), d_left(pl, SLOT_MSA_LEFT);
    int rc;
    if ((rc = msa_upload(pl, SLOT_MSA_ROWS, row_ids, (size_t)n_rows * 4)) || (rc = msa_upload(pl, SLOT_MSA_OPS, ops, (size_t)n_ops * 4)) ||
        (rc = msa_upload(pl, SLOT_MSA_OPTR, ops_ptr, (size_t)(n_rows + 1) * 8)) || (rc = msa_upload(pl, SLOT_MSA_PART, part_of_row.data(), (size_t)n_rows * 4)) ||
        (rc = msa_upload(pl, SLOT_MSA_FIRST, first_row, (size_t)(n_parts + 1) * 4)) || (rc = msa_upload(pl, SLOT_MSA_LM, Lm.data(), (size_t)n_parts * 4)) ||
        (rc = msa_upload(pl, SLOT_MSA_SBASE, slot_base.data(), (size_t)(n_parts + 1) * 4)) || (rc = d_longest.alloc((size_t)n_slots * 4)) ||
        (rc = d_width.alloc((size_t)n_slots * 4)) || (rc = d_cslot.alloc((size_t)n_slots * 4)) || (rc = d_tot.alloc(32)) ||
        (rc = d_wide.alloc((size_t)std::max<uint64_t>(wide_cap, 1) * 32)) || (rc = d_ncols.alloc((size_t)n_parts * 4)))
        return rc;
    if (placed && ((rc = d_widx.alloc((size_t)n_slots * 4)) || (rc = d_left.alloc((size_t)std::max<uint64_t>(placed->left_cap, 1) * 32)))) return rc;
    const uint32_t *d_rows = msa_slot<uint32_t>(pl, SLOT_MSA_ROWS), *d_ops = msa_slot<uint32_t>(pl, SLOT_MSA_OPS);
    const unsigned long long *d_optr = msa_slot<unsigned long long>(pl, SLOT_MSA_OPTR);
    ISO_HIP_CHECK(hipMemsetAsync(d_longest.p, 0, (size_t)n_slots * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, 32, 0));
    uint32_t *tot = d_tot.as<uint32_t>();          // [0] wide slots placed on the device, [2] bad flag, [4..5] wide records, [6..7] left-over records (64 bit)
    MsaBatch B = msa_batch_desc(pl, n_parts, n_rows);          // (m_off and col_base follow the layout)
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_msa_ops_scan, dim3((n_rows + 255) / 256), dim3(256), 0, 0, s->dev, B, d_rows, d_ops, d_optr, d_longest.as<uint32_t>(), tot + 2);
    hipLaunchKernelGGL(k_msa_layout, dim3(n_parts), dim3(1024), 0, 0, B, d_longest.as<uint32_t>(), d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), d_ncols.as<uint32_t>());
    if (placed) hipLaunchKernelGGL(k_msa_wide_number, dim3((n_slots + 255) / 256), dim3(256), 0, 0, d_longest.as<uint32_t>(), n_slots, d_widx.as<uint32_t>(), tot);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    uint32_t h_tot[4];
    ISO_HIP_CHECK(hipMemcpy(h_tot, d_tot.p, 16, hipMemcpyDeviceToHost));
    if (h_tot[2]) { g_last_error = "the ops of a row do not spell the centre and the member"; return ISOCON_E_ARG; }
    H.ncols.resize(n_parts);
    ISO_HIP_CHECK(copy_d2h(H.ncols.data(), d_ncols.p, (size_t)n_parts * 4));
    H.m_off.assign((size_t)n_parts + 1, 0);
    H.col_base.assign((size_t)n_parts + 1, 0);
    H.first_row.assign(first_row, first_row + n_parts + 1);
    for (uint32_t p = 0; p < n_parts; ++p) {
        H.m_off[p + 1] = H.m_off[p] + (unsigned long long)(first_row[p + 1] - first_row[p]) * H.ncols[p];
        if ((uint64_t)H.col_base[p] + H.ncols[p] > 0xffffffffull) { g_last_error = "too many columns in one batch"; return ISOCON_E_UNSUPPORTED; }
        H.col_base[p + 1] = H.col_base[p] + H.ncols[p];
        out_n_cols[p] = H.ncols[p];
    }
    const size_t cells = (size_t)H.m_off[n_parts];
    if ((rc = d_M.alloc(std::max<size_t>(cells, 16))) || (rc = msa_upload(pl, SLOT_MSA_MOFF, H.m_off.data(), (size_t)(n_parts + 1) * 8)) ||
        (rc = msa_upload(pl, SLOT_MSA_CBASE, H.col_base.data(), (size_t)(n_parts + 1) * 4)))
        return rc;
    ISO_HIP_CHECK(hipMemsetAsync(d_M.p, '-', cells, 0));
    const uint32_t n_wide_slots = placed ? h_tot[0] : 0u;
    if (placed) {
        if ((rc = d_keys.alloc((size_t)std::max<uint32_t>(n_wide_slots, 1) * 16))) return rc;
        ISO_HIP_CHECK(hipMemsetAsync(d_keys.p, 0xff, (size_t)n_wide_slots * 16, 0));          // PLACE_KEY_NONE
    }
    B = msa_batch_desc(pl, n_parts, n_rows);
    tm.start();
    hipLaunchKernelGGL(k_msa_fill, dim3((n_rows + 3) / 4), dim3(256), 0, 0, s->dev, B, d_rows, d_ops, d_optr, d_longest.as<uint32_t>(),
                       d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), d_M.as<uint8_t>(), d_wide.as<uint32_t>(), (unsigned long long)wide_cap,
                       reinterpret_cast<unsigned long long *>(tot + 4));
    if (placed && wide_cap && n_wide_slots) {          // (grids by the upper bound: a thread or wave beyond the records that were listed ends at once)
        unsigned long long *cnt_w = reinterpret_cast<unsigned long long *>(tot + 4), *cnt_l = reinterpret_cast<unsigned long long *>(tot + 6);
        const unsigned long long lcap = placed->left_cap;
        hipLaunchKernelGGL(k_msa_slot_rep<1>, dim3((unsigned)((wide_cap + 255) / 256)), dim3(256), 0, 0, s->dev, B, d_rows, d_longest.as<uint32_t>(), d_widx.as<uint32_t>(),
                           d_wide.as<uint32_t>(), (unsigned long long)wide_cap, cnt_w, d_keys.as<unsigned long long>(), d_left.as<uint32_t>(), lcap, cnt_l);
        hipLaunchKernelGGL(k_msa_slot_rep<2>, dim3((unsigned)((wide_cap + 255) / 256)), dim3(256), 0, 0, s->dev, B, d_rows, d_longest.as<uint32_t>(), d_widx.as<uint32_t>(),
                           d_wide.as<uint32_t>(), (unsigned long long)wide_cap, cnt_w, d_keys.as<unsigned long long>(), d_left.as<uint32_t>(), lcap, cnt_l);
        hipLaunchKernelGGL(k_msa_place, dim3((unsigned)((wide_cap + 3) / 4)), dim3(256), 0, 0, s->dev, B, d_rows, d_longest.as<uint32_t>(), d_cslot.as<uint32_t>(),
                           d_widx.as<uint32_t>(), d_keys.as<unsigned long long>(), d_wide.as<uint32_t>(), (unsigned long long)wide_cap, cnt_w, d_M.as<uint8_t>());
    }
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    unsigned long long cnt[2] = {0, 0};          // records listed; of them left to the host
    ISO_HIP_CHECK(hipMemcpy(cnt, tot + 4, 16, hipMemcpyDeviceToHost));
    bool too_small = false;
    if (placed) {
        if (cnt[0] > wide_cap) { g_last_error = "more wide-slot records than code-3 ops"; return ISOCON_E_ARG; }
        if (!n_wide_slots) cnt[1] = cnt[0];          // (no slot for the device: every record is left; listed below)
        *placed->n_left = cnt[1];
        *placed->n_placed = cnt[0] - cnt[1];
        too_small = cnt[1] > placed->left_cap;          // (the matrix is built all the same: the caller calls again for the list)
        if (!too_small && cnt[1]) ISO_HIP_CHECK(copy_d2h(placed->out_left, n_wide_slots ? d_left.p : d_wide.p, (size_t)cnt[1] * 32));
    } else {
        *n_wide = cnt[0];
        if (cnt[0] > wide_cap) return ISOCON_E_CAPACITY;          // (call again with room for *n_wide records)
        if (cnt[0]) ISO_HIP_CHECK(copy_d2h(out_wide, d_wide.p, (size_t)cnt[0] * 32));
    }
    if (out_col_slot) ISO_HIP_CHECK(copy_d2h(out_col_slot, d_cslot.p, (size_t)n_slots * 4));
    if (out_longest) ISO_HIP_CHECK(copy_d2h(out_longest, d_longest.p, (size_t)n_slots * 4));
    H.by = by;
    H.serial = s->serial;
    H.n_parts = n_parts;
    H.n_rows = n_rows;
    return too_small ? ISOCON_E_CAPACITY : ISOCON_OK;
}

// nullptr, or what is wrong with the first patch that does not lie inside its row's matrix
const char *msa_patch_fault(const MsaBuilt &H, const uint32_t *patch_row, const uint32_t *patch_col, const uint32_t *patch_ptr, uint32_t n_patches)
{
    for (uint32_t i = 0; i < n_patches; ++i) {
        if (patch_row[i] >= H.n_rows || patch_ptr[i + 1] < patch_ptr[i]) return "patch outside the batch";
        const uint32_t p = (uint32_t)(std::upper_bound(H.first_row.begin(), H.first_row.end(), patch_row[i]) - H.first_row.begin()) - 1;
        if ((uint64_t)patch_col[i] + (patch_ptr[i + 1] - patch_ptr[i]) > H.ncols[p]) return "patch outside its matrix";
    }
    return nullptr;
}

// The correction proper on the matrices H describes (in SLOT_MSA_IN of pl, their tables in the slots of msa_batch_desc): the patches (checked
// by the caller), column statistics, per-row correction with the list of list_cap positions in LDS (MSA_BATCH_CAND or MSA_MAX_CAND) and, with
// hbm_repeat, once more with the list in HBM for the rows that have more; gap stripping; results to the host.  out_class_totals: partition 0's.
int msa_correct_built(ScratchPool *pl, const MsaBuilt &H, const uint32_t *patch_row, const uint32_t *patch_col, const uint32_t *patch_ptr, const uint8_t *patch_bytes,
                      uint32_t n_patches, const int32_t *degree, int list_cap, bool hbm_repeat, uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets,
                      int32_t *out_n_cand, int64_t *out_class_totals, float *kernel_ms)
{
    const uint32_t n_parts = H.n_parts, n_rows = H.n_rows;
    const MsaBatch B = msa_batch_desc(pl, n_parts, n_rows);
    uint8_t *d_M = msa_slot<uint8_t>(pl, SLOT_MSA_IN);
    const size_t cells = (size_t)H.m_off[n_parts];
    const uint32_t n_colsum = H.col_base[n_parts];
    int rc;
    if (n_patches) {
        const size_t nb = patch_ptr[n_patches];
        if ((rc = msa_upload(pl, SLOT_MSA_PROW, patch_row, (size_t)n_patches * 4)) || (rc = msa_upload(pl, SLOT_MSA_PCOL, patch_col, (size_t)n_patches * 4)) ||
            (rc = msa_upload(pl, SLOT_MSA_PPTR, patch_ptr, (size_t)(n_patches + 1) * 4)) || (rc = msa_upload(pl, SLOT_MSA_PBYTES, patch_bytes, nb)))
            return rc;
        hipLaunchKernelGGL(k_msa_patch, dim3((n_patches + 3) / 4), dim3(256), 0, 0, d_M, B, msa_slot<uint32_t>(pl, SLOT_MSA_PROW), msa_slot<uint32_t>(pl, SLOT_MSA_PCOL),
                           msa_slot<uint32_t>(pl, SLOT_MSA_PPTR), msa_slot<uint8_t>(pl, SLOT_MSA_PBYTES), n_patches);
        ISO_HIP_CHECK(hipGetLastError());
    }
    // the column blocks of all partitions, and the same cut into chunks of MSA_ROWS_PER_WG rows for the counting launch
    std::vector<uint32_t> cb_part, cb_col0, cbr;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const uint32_t nr = H.first_row[p + 1] - H.first_row[p];
        for (uint32_t c0 = 0; c0 < H.ncols[p]; c0 += 256) {
            cb_part.push_back(p); cb_col0.push_back(c0);
            for (uint32_t r0 = 0; r0 < nr; r0 += MSA_ROWS_PER_WG) { cbr.push_back(p); cbr.push_back(c0); cbr.push_back(r0); }
        }
    }
    DevBuf d_out(pl, SLOT_MSA_OUT), d_counts(pl, SLOT_MSA_COUNTS), d_maj(pl, SLOT_MSA_MAJ), d_flags(pl, SLOT_MSA_FLAGS), d_tot(pl, SLOT_MSA_TOT), d_ncand(pl, SLOT_MSA_NCAND),
        d_len(pl, SLOT_MSA_LEN), d_packed(pl, SLOT_MSA_PACKED);
    const size_t counts_bytes = (size_t)5 * std::max<uint32_t>(n_colsum, 1) * 4;
    if ((rc = d_out.alloc(std::max<size_t>(cells, 16))) || (rc = msa_upload(pl, SLOT_MSA_DEG, degree, (size_t)n_rows * 4)) || (rc = d_counts.alloc(counts_bytes)) ||
        (rc = d_maj.alloc(std::max<uint32_t>(n_colsum, 1))) || (rc = d_flags.alloc(std::max<uint32_t>(n_colsum, 1))) || (rc = d_tot.alloc((size_t)24 * n_parts)) ||
        (rc = d_ncand.alloc((size_t)n_rows * 4)) || (rc = d_len.alloc((size_t)n_rows * 4)) || (rc = msa_upload(pl, SLOT_MSA_CBP, cb_part.data(), cb_part.size() * 4)) ||
        (rc = msa_upload(pl, SLOT_MSA_CBC, cb_col0.data(), cb_col0.size() * 4)) || (rc = msa_upload(pl, SLOT_MSA_CBR, cbr.data(), cbr.size() * 4)))
        return rc;
    const int32_t *d_deg = msa_slot<int32_t>(pl, SLOT_MSA_DEG);
    ISO_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, (size_t)24 * n_parts, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, counts_bytes, 0));
    const auto k_row_correct_lds = list_cap == MSA_MAX_CAND ? k_msa_row_correct<MSA_MAX_CAND> : k_msa_row_correct<MSA_BATCH_CAND>;
    EventTimer tm;
    tm.start();
    if (!cbr.empty())
        hipLaunchKernelGGL(k_msa_col_counts, dim3((unsigned)(cbr.size() / 3)), dim3(256), 0, 0, d_M, B, msa_slot<uint32_t>(pl, SLOT_MSA_CBR), d_deg, d_counts.as<int32_t>());
    if (!cb_part.empty())
        hipLaunchKernelGGL(k_msa_col_finish, dim3((unsigned)cb_part.size()), dim3(256), 0, 0, B, msa_slot<uint32_t>(pl, SLOT_MSA_CBP), msa_slot<uint32_t>(pl, SLOT_MSA_CBC),
                           d_counts.as<int32_t>(), d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>());
    hipLaunchKernelGGL(k_row_correct_lds, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_M, d_out.as<uint8_t>(), B, d_deg, d_counts.as<int32_t>(), d_maj.as<uint8_t>(),
                       d_flags.as<uint8_t>(), d_tot.as<unsigned long long>(), d_ncand.as<int32_t>(), (const uint32_t *)nullptr, 0u, (double *)nullptr, (uint32_t *)nullptr, 0u);
    hipLaunchKernelGGL(k_msa_row_lengths, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), B, d_len.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    ISO_HIP_CHECK(copy_d2h(out_n_cand, d_ncand.p, (size_t)n_rows * 4));
    // rows whose list of correctable positions did not fit the LDS: once more, list in HBM (and their lengths again)
    std::vector<uint32_t> big;
    for (uint32_t r = 0; hbm_repeat && r < n_rows; ++r) if (out_n_cand[r] < 0) big.push_back(r);
    if (!big.empty()) {
        const uint32_t stride = *std::max_element(H.ncols.begin(), H.ncols.end());
        DevBuf d_list, d_freq, d_col;
        if ((rc = d_list.alloc(big.size() * 4)) || (rc = d_freq.alloc(big.size() * (size_t)stride * 8)) || (rc = d_col.alloc(big.size() * (size_t)stride * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_list.p, big.data(), big.size() * 4));
        tm.start();
        hipLaunchKernelGGL(k_msa_row_correct<MSA_LIST_HBM>, dim3(((uint32_t)big.size() + 3) / 4), dim3(256), 0, 0, d_M, d_out.as<uint8_t>(), B, d_deg, d_counts.as<int32_t>(),
                           d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>(), d_ncand.as<int32_t>(), d_list.as<uint32_t>(), (uint32_t)big.size(),
                           d_freq.as<double>(), d_col.as<uint32_t>(), stride);
        hipLaunchKernelGGL(k_msa_row_lengths, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), B, d_len.as<uint32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(hipDeviceSynchronize());      // d_freq / d_col are freed when this scope ends
        ISO_HIP_CHECK(copy_d2h(out_n_cand, d_ncand.p, (size_t)n_rows * 4));
    }
    std::vector<uint32_t> len(n_rows);
    ISO_HIP_CHECK(copy_d2h(len.data(), d_len.p, (size_t)n_rows * 4));
    if (out_class_totals) {
        unsigned long long t[3];
        ISO_HIP_CHECK(hipMemcpy(t, d_tot.p, 24, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3; ++i) out_class_totals[i] = (int64_t)t[i];
    }
    out_offsets[0] = 0;
    for (uint32_t r = 0; r < n_rows; ++r) out_offsets[r + 1] = out_offsets[r] + len[r];
    const uint64_t total = out_offsets[n_rows];
    if (total > packed_cap) return ISOCON_E_CAPACITY;
    if ((rc = d_packed.alloc(total)) || (rc = msa_upload(pl, SLOT_MSA_OFF, out_offsets, (size_t)(n_rows + 1) * 8))) return rc;
    tm.start();
    hipLaunchKernelGGL(k_msa_strip, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), B, msa_slot<uint64_t>(pl, SLOT_MSA_OFF), d_packed.as<uint8_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (total) ISO_HIP_CHECK(copy_d2h(out_packed, d_packed.p, total));
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

// the build of this store and shape by `by`, or nullptr
MsaBuilt *msa_built(isocon_store *s, MsaBuilt::By by, uint32_t n_parts, uint32_t n_rows)
{
    MsaBuilt &H = s->pool.msa;
    return H.by == by && H.serial == s->serial && H.n_parts == n_parts && H.n_rows == n_rows ? &H : nullptr;
}

}  // namespace

// a matrix of the host: uploaded as a batch of one partition into the process' pool (no store is needed)
extern "C" int isocon_msa_correct(const uint8_t *matrix, uint32_t n_rows, uint32_t n_cols, const int32_t *degree,
                                  uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                                  int64_t *out_class_totals, float *kernel_ms)
{
    if (!matrix || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_rows == 0 || n_cols == 0) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    ScratchPool *pl = &g_scratch;
    pl->msa = MsaBuilt();          // (a build in this pool loses its slots)
    MsaBuilt H;
    H.n_parts = 1;
    H.n_rows = n_rows;
    H.ncols = {n_cols};
    H.col_base = {0, n_cols};
    H.first_row = {0, n_rows};
    H.m_off = {0, (unsigned long long)n_rows * n_cols};
    DevBuf d_part(pl, SLOT_MSA_PART);
    int rc;
    if ((rc = msa_upload(pl, SLOT_MSA_IN, matrix, (size_t)H.m_off[1])) || (rc = d_part.alloc((size_t)n_rows * 4)) || (rc = msa_upload(pl, SLOT_MSA_FIRST, H.first_row.data(), 8)) ||
        (rc = msa_upload(pl, SLOT_MSA_NCOLS, H.ncols.data(), 4)) || (rc = msa_upload(pl, SLOT_MSA_MOFF, H.m_off.data(), 16)) ||
        (rc = msa_upload(pl, SLOT_MSA_CBASE, H.col_base.data(), 8)))
        return rc;
    ISO_HIP_CHECK(hipMemsetAsync(d_part.p, 0, (size_t)n_rows * 4, 0));
    return msa_correct_built(pl, H, nullptr, nullptr, nullptr, nullptr, 0, degree, MSA_MAX_CAND, true, out_packed, packed_cap, out_offsets, out_n_cand, out_class_totals, kernel_ms);
}

extern "C" int isocon_msa_build_ops(isocon_store *s, uint32_t n_rows, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
                                    uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide, uint64_t wide_cap,
                                    uint64_t *n_wide, float *kernel_ms)
{
    if (!s || !row_ids || !ops_ptr || !out_n_cols || !n_wide || n_rows == 0 || (wide_cap && !out_wide)) return ISOCON_E_ARG;
    const uint32_t first_row[2] = {0, n_rows};
    return msa_build(s, MsaBuilt::SINGLE, 1, first_row, row_ids, ops, ops_ptr, out_n_cols, out_col_slot, out_longest, out_wide, wide_cap, n_wide, kernel_ms);
}

extern "C" int isocon_msa_build_ops_placed(isocon_store *s, uint32_t n_rows, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
                                           uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_left, uint64_t left_cap,
                                           uint64_t *n_left, uint64_t *n_placed, float *kernel_ms)
{
    if (!s || !row_ids || !ops_ptr || !out_n_cols || !n_left || !n_placed || n_rows == 0 || (left_cap && !out_left)) return ISOCON_E_ARG;
    const uint32_t first_row[2] = {0, n_rows};
    const MsaPlaced placed = {out_left, left_cap, n_left, n_placed};
    return msa_build(s, MsaBuilt::SINGLE, 1, first_row, row_ids, ops, ops_ptr, out_n_cols, out_col_slot, out_longest, nullptr, 0, nullptr, kernel_ms, &placed);
}

extern "C" int isocon_msa_correct_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, const uint32_t *patch_row, const uint32_t *patch_col,
                                        const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                                        uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                                        int64_t *out_class_totals, float *kernel_ms)
{
    if (!s || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_rows == 0 || n_cols == 0 ||
        (n_patches && (!patch_row || !patch_col || !patch_ptr || !patch_bytes)))
        return ISOCON_E_ARG;
    MsaBuilt *H = msa_built(s, MsaBuilt::SINGLE, 1, n_rows);
    if (!H || H->ncols[0] != n_cols) {
        g_last_error = "no matrix of this shape was built for this store (isocon_msa_build_ops comes first)";
        return ISOCON_E_ARG;
    }
    if (kernel_ms) *kernel_ms = 0.f;
    if (msa_patch_fault(*H, patch_row, patch_col, patch_ptr, n_patches)) { g_last_error = "patch outside the matrix"; return ISOCON_E_ARG; }
    H->by = MsaBuilt::NONE;          // (the correction leaves the matrix as it is, but one build serves one correction)
    return msa_correct_built(&s->pool, *H, patch_row, patch_col, patch_ptr, patch_bytes, n_patches, degree, MSA_MAX_CAND, true, out_packed, packed_cap, out_offsets, out_n_cand,
                             out_class_totals, kernel_ms);
}

// the built matrix, for tests (rows as the reference's create_multialignment_matrix would give them)
extern "C" int isocon_msa_read_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, uint8_t *out_matrix)
{
    if (!s || !out_matrix) return ISOCON_E_ARG;
    const MsaBuilt *H = msa_built(s, MsaBuilt::SINGLE, 1, n_rows);
    if (!H || H->ncols[0] != n_cols) return ISOCON_E_ARG;
    ISO_HIP_CHECK(copy_d2h(out_matrix, s->pool.slots[SLOT_MSA_IN].p, (size_t)n_rows * n_cols));
    return ISOCON_OK;
}

extern "C" int isocon_msa_build_ops_batch(isocon_store *s, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops,
                                          const uint64_t *ops_ptr, uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide,
                                          uint64_t wide_cap, uint64_t *n_wide, float *kernel_ms)
{
    if (!s || !first_row || !row_ids || !ops_ptr || !out_n_cols || !n_wide || n_parts == 0 || (wide_cap && !out_wide)) return ISOCON_E_ARG;
    return msa_build(s, MsaBuilt::BATCH, n_parts, first_row, row_ids, ops, ops_ptr, out_n_cols, out_col_slot, out_longest, out_wide, wide_cap, n_wide, kernel_ms);
}

extern "C" int isocon_msa_build_ops_placed_batch(isocon_store *s, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops,
                                                 const uint64_t *ops_ptr, uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_left,
                                                 uint64_t left_cap, uint64_t *n_left, uint64_t *n_placed, float *kernel_ms)
{
    if (!s || !first_row || !row_ids || !ops_ptr || !out_n_cols || !n_left || !n_placed || n_parts == 0 || (left_cap && !out_left)) return ISOCON_E_ARG;
    const MsaPlaced placed = {out_left, left_cap, n_left, n_placed};
    return msa_build(s, MsaBuilt::BATCH, n_parts, first_row, row_ids, ops, ops_ptr, out_n_cols, out_col_slot, out_longest, nullptr, 0, nullptr, kernel_ms, &placed);
}

// a row with more than MSA_BATCH_CAND correctable positions keeps n_cand = -1: the caller corrects its partition through the single-partition entries
extern "C" int isocon_msa_correct_built_batch(isocon_store *s, uint32_t n_parts, uint32_t n_rows, const uint32_t *patch_row, const uint32_t *patch_col,
                                              const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                                              uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand, float *kernel_ms)
{
    if (!s || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_parts == 0 || n_rows == 0 ||
        (n_patches && (!patch_row || !patch_col || !patch_ptr || !patch_bytes)))
        return ISOCON_E_ARG;
    MsaBuilt *H = msa_built(s, MsaBuilt::BATCH, n_parts, n_rows);
    if (!H) {
        g_last_error = "no batch of this shape was built for this store (isocon_msa_build_ops_batch comes first)";
        return ISOCON_E_ARG;
    }
    if (kernel_ms) *kernel_ms = 0.f;
    H->by = MsaBuilt::NONE;
    if (const char *fault = msa_patch_fault(*H, patch_row, patch_col, patch_ptr, n_patches)) { g_last_error = fault; return ISOCON_E_ARG; }
    const int rc = msa_correct_built(&s->pool, *H, patch_row, patch_col, patch_ptr, patch_bytes, n_patches, degree, MSA_BATCH_CAND, false, out_packed, packed_cap, out_offsets,
                                     out_n_cand, nullptr, kernel_ms);
    if (rc == ISOCON_E_CAPACITY) H->by = MsaBuilt::BATCH;          // (the built matrices are still there: call again with room)
    return rc;
}
