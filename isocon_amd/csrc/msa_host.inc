// msa_host.inc -- host side of isocon_msa_correct (included by isocon_hip.hip).

namespace {

// The correction proper on a matrix that is in device memory (d_M: n_rows x n_cols bytes): column statistics, per-row correction,
// gap stripping; results to the host.
int msa_correct_core(const uint8_t *d_M, uint32_t n_rows, uint32_t n_cols, const int32_t *degree, uint8_t *out_packed, uint64_t packed_cap,
                     uint64_t *out_offsets, int32_t *out_n_cand, int64_t *out_class_totals, float *kernel_ms)
{
    const size_t cells = (size_t)n_rows * n_cols;
    ScratchPool *pl = &g_scratch;
    DevBuf d_out(pl, SLOT_MSA_OUT), d_deg(pl, SLOT_MSA_DEG), d_counts(pl, SLOT_MSA_COUNTS), d_maj(pl, SLOT_MSA_MAJ),
        d_flags(pl, SLOT_MSA_FLAGS), d_tot(pl, SLOT_MSA_TOT), d_ncand(pl, SLOT_MSA_NCAND), d_len(pl, SLOT_MSA_LEN), d_off(pl, SLOT_MSA_OFF),
        d_packed(pl, SLOT_MSA_PACKED);
    int rc;
    if ((rc = d_out.alloc(cells)) || (rc = d_deg.alloc((size_t)n_rows * 4)) || (rc = d_counts.alloc((size_t)5 * n_cols * 4)) ||
        (rc = d_maj.alloc(n_cols)) || (rc = d_flags.alloc(n_cols)) || (rc = d_tot.alloc(24)) || (rc = d_ncand.alloc((size_t)n_rows * 4)) ||
        (rc = d_len.alloc((size_t)n_rows * 4)) || (rc = d_off.alloc((size_t)(n_rows + 1) * 8)))
        return rc;
    ISO_HIP_CHECK(copy_h2d(d_deg.p, degree, (size_t)n_rows * 4));
    ISO_HIP_CHECK(hipMemset(d_tot.p, 0, 24));
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_msa_col_stats, dim3((n_cols + 255) / 256), dim3(256), 0, 0, d_M, n_rows, n_cols, d_deg.as<int32_t>(),
                       d_counts.as<int32_t>(), d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>());
    hipLaunchKernelGGL(k_msa_row_correct<false>, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_M, d_out.as<uint8_t>(), n_rows, n_cols,
                       d_deg.as<int32_t>(), d_counts.as<int32_t>(), d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>(),
                       d_ncand.as<int32_t>(), (const uint32_t *)nullptr, 0u, (double *)nullptr, (uint32_t *)nullptr);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    ISO_HIP_CHECK(copy_d2h(out_n_cand, d_ncand.p, (size_t)n_rows * 4));
    // rows whose list of correctable positions did not fit the LDS (more than MSA_MAX_CAND): once more, list in HBM
    std::vector<uint32_t> big;
    for (uint32_t r = 0; r < n_rows; ++r) if (out_n_cand[r] < 0) big.push_back(r);
    if (!big.empty()) {
        DevBuf d_list, d_freq, d_col;
        if ((rc = d_list.alloc(big.size() * 4)) || (rc = d_freq.alloc(big.size() * (size_t)n_cols * 8)) || (rc = d_col.alloc(big.size() * (size_t)n_cols * 4)))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_list.p, big.data(), big.size() * 4));
        tm.start();
        hipLaunchKernelGGL(k_msa_row_correct<true>, dim3(((uint32_t)big.size() + 3) / 4), dim3(256), 0, 0, d_M, d_out.as<uint8_t>(), n_rows,
                           n_cols, d_deg.as<int32_t>(), d_counts.as<int32_t>(), d_maj.as<uint8_t>(), d_flags.as<uint8_t>(),
                           d_tot.as<unsigned long long>(), d_ncand.as<int32_t>(), d_list.as<uint32_t>(), (uint32_t)big.size(), d_freq.as<double>(),
                           d_col.as<uint32_t>());
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        ISO_HIP_CHECK(hipDeviceSynchronize());      // d_freq / d_col are freed when this scope ends
        ISO_HIP_CHECK(copy_d2h(out_n_cand, d_ncand.p, (size_t)n_rows * 4));
    }
    tm.start();
    hipLaunchKernelGGL(k_msa_row_lengths, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), n_rows, n_cols, d_len.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
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
    if ((rc = d_packed.alloc(total ? total : 16))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_off.p, out_offsets, (size_t)(n_rows + 1) * 8));
    tm.start();
    hipLaunchKernelGGL(k_msa_strip, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), n_rows, n_cols, d_off.as<uint64_t>(), d_packed.as<uint8_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (total) ISO_HIP_CHECK(copy_d2h(out_packed, d_packed.p, total));
    if (kernel_ms) *kernel_ms += tm.total;
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_msa_correct(const uint8_t *matrix, uint32_t n_rows, uint32_t n_cols, const int32_t *degree,
                                  uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                                  int64_t *out_class_totals, float *kernel_ms)
{
    if (!matrix || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_rows == 0 || n_cols == 0) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    const size_t cells = (size_t)n_rows * n_cols;
    DevBuf d_M(&g_scratch, SLOT_MSA_IN);
    int rc;
    if ((rc = d_M.alloc(cells))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_M.p, matrix, cells));
    return msa_correct_core(d_M.as<uint8_t>(), n_rows, n_cols, degree, out_packed, packed_cap, out_offsets, out_n_cand, out_class_totals, kernel_ms);
}

// ---- the matrix built on the device from CIGAR ops (msa_build.hpp) ------------------------------------------------------------------
extern "C" int isocon_msa_build_ops(isocon_store *s, uint32_t n_rows, const uint32_t *row_ids, const uint32_t *ops, const uint64_t *ops_ptr,
                                    uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide, uint64_t wide_cap,
                                    uint64_t *n_wide, float *kernel_ms)
{
    if (!s || !row_ids || !ops_ptr || !out_n_cols || !n_wide || n_rows == 0 || (wide_cap && !out_wide)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!s->acgt) { g_last_error = "the consensus correction needs a store over the alphabet ACGT"; return ISOCON_E_ALPHABET; }
    const uint32_t n = s->dev.n;
    for (uint32_t r = 0; r < n_rows; ++r)
        if (row_ids[r] >= n) { g_last_error = "row id out of range"; return ISOCON_E_ARG; }
    if (ops_ptr[0] != 0 || ops_ptr[1] != 0) { g_last_error = "row 0 is the centre: it has no ops"; return ISOCON_E_ARG; }
    for (uint32_t r = 0; r < n_rows; ++r)
        if (ops_ptr[r + 1] < ops_ptr[r]) return ISOCON_E_ARG;
    const uint64_t n_ops = ops_ptr[n_rows];
    if (n_ops && !ops) return ISOCON_E_ARG;
    const uint32_t Lm = (uint32_t)s->lens[row_ids[0]];
    ScratchPool *pl = &s->pool;
    pl->msa_tag = MsaTag();
    pl->msab.valid = false;          // (the batched build shares these slots)
    DevBuf d_rows(pl, SLOT_MSA_ROWS), d_ops(pl, SLOT_MSA_OPS), d_optr(pl, SLOT_MSA_OPTR), d_longest(pl, SLOT_MSA_LONGEST), d_width(pl, SLOT_MSA_WIDTH),
        d_cslot(pl, SLOT_MSA_CSLOT), d_tot(pl, SLOT_MSA_LTOT), d_wide(pl, SLOT_MSA_WIDE), d_M(pl, SLOT_MSA_IN);
    int rc;
    if ((rc = d_rows.alloc((size_t)n_rows * 4)) || (rc = d_ops.alloc((size_t)std::max<uint64_t>(n_ops, 1) * 4)) || (rc = d_optr.alloc((size_t)(n_rows + 1) * 8)) ||
        (rc = d_longest.alloc((size_t)(Lm + 1) * 4)) || (rc = d_width.alloc((size_t)(Lm + 1) * 4)) || (rc = d_cslot.alloc((size_t)(Lm + 1) * 4)) ||
        (rc = d_tot.alloc(32)) || (rc = d_wide.alloc((size_t)std::max<uint64_t>(wide_cap, 1) * 32)))
        return rc;
    ISO_HIP_CHECK(copy_h2d(d_rows.p, row_ids, (size_t)n_rows * 4));
    if (n_ops) ISO_HIP_CHECK(copy_h2d(d_ops.p, ops, (size_t)n_ops * 4));
    ISO_HIP_CHECK(copy_h2d(d_optr.p, ops_ptr, (size_t)(n_rows + 1) * 8));
    ISO_HIP_CHECK(hipMemsetAsync(d_longest.p, 0, (size_t)(Lm + 1) * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, 32, 0));
    EventTimer tm;
    tm.start();
    uint32_t *tot = d_tot.as<uint32_t>();          // [0] columns, [1] wide slots, [2] bad flag, [4..5] wide entries (64 bit)
    hipLaunchKernelGGL(k_msa_ops_scan, dim3((n_rows + 255) / 256), dim3(256), 0, 0, s->dev, d_rows.as<uint32_t>(), n_rows, d_ops.as<uint32_t>(),
                       d_optr.as<unsigned long long>(), Lm, d_longest.as<uint32_t>(), tot + 2);
    hipLaunchKernelGGL(k_msa_layout, dim3(1), dim3(1024), 0, 0, d_longest.as<uint32_t>(), Lm, d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), tot);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    uint32_t h_tot[4];
    ISO_HIP_CHECK(hipMemcpy(h_tot, d_tot.p, 16, hipMemcpyDeviceToHost));
    if (h_tot[2]) { g_last_error = "the ops of a row do not spell the centre and the member"; return ISOCON_E_ARG; }
    const uint32_t n_cols = h_tot[0];
    *out_n_cols = n_cols;
    const size_t cells = (size_t)n_rows * n_cols;
    if ((rc = d_M.alloc(std::max<size_t>(cells, 16)))) return rc;
    ISO_HIP_CHECK(hipMemsetAsync(d_M.p, '-', cells, 0));
    tm.start();
    hipLaunchKernelGGL(k_msa_fill, dim3((n_rows + 3) / 4), dim3(256), 0, 0, s->dev, d_rows.as<uint32_t>(), n_rows, d_ops.as<uint32_t>(),
                       d_optr.as<unsigned long long>(), Lm, d_longest.as<uint32_t>(), d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), n_cols, d_M.as<uint8_t>(),
                       d_wide.as<uint32_t>(), (unsigned long long)wide_cap, reinterpret_cast<unsigned long long *>(tot + 4));
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    unsigned long long cnt = 0;
    ISO_HIP_CHECK(hipMemcpy(&cnt, tot + 4, 8, hipMemcpyDeviceToHost));
    *n_wide = cnt;
    if (cnt > wide_cap) return ISOCON_E_CAPACITY;          // (call again with room for *n_wide entries)
    if (cnt) ISO_HIP_CHECK(copy_d2h(out_wide, d_wide.p, (size_t)cnt * 32));
    if (out_col_slot) ISO_HIP_CHECK(copy_d2h(out_col_slot, d_cslot.p, (size_t)(Lm + 1) * 4));
    if (out_longest) ISO_HIP_CHECK(copy_d2h(out_longest, d_longest.p, (size_t)(Lm + 1) * 4));
    pl->msa_tag.valid = true;
    pl->msa_tag.serial = s->serial;
    pl->msa_tag.n_rows = n_rows;
    pl->msa_tag.n_cols = n_cols;
    return ISOCON_OK;
}

extern "C" int isocon_msa_correct_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, const uint32_t *patch_row, const uint32_t *patch_col,
                                        const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                                        uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand,
                                        int64_t *out_class_totals, float *kernel_ms)
{
    if (!s || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_rows == 0 || n_cols == 0 ||
        (n_patches && (!patch_row || !patch_col || !patch_ptr || !patch_bytes)))
        return ISOCON_E_ARG;
    ScratchPool *pl = &s->pool;
    if (!pl->msa_tag.valid || pl->msa_tag.serial != s->serial || pl->msa_tag.n_rows != n_rows || pl->msa_tag.n_cols != n_cols) {
        g_last_error = "no matrix of this shape was built for this store (isocon_msa_build_ops comes first)";
        return ISOCON_E_ARG;
    }
    if (kernel_ms) *kernel_ms = 0.f;
    uint8_t *d_M = static_cast<uint8_t *>(pl->slots[SLOT_MSA_IN].p);
    if (n_patches) {
        for (uint32_t i = 0; i < n_patches; ++i)
            if (patch_row[i] >= n_rows || patch_ptr[i + 1] < patch_ptr[i] || (uint64_t)patch_col[i] + (patch_ptr[i + 1] - patch_ptr[i]) > n_cols) {
                g_last_error = "patch outside the matrix";
                return ISOCON_E_ARG;
            }
        DevBuf d_pr(pl, SLOT_MSA_PROW), d_pc(pl, SLOT_MSA_PCOL), d_pp(pl, SLOT_MSA_PPTR), d_pb(pl, SLOT_MSA_PBYTES);
        int rc;
        const size_t nb = patch_ptr[n_patches];
        if ((rc = d_pr.alloc((size_t)n_patches * 4)) || (rc = d_pc.alloc((size_t)n_patches * 4)) || (rc = d_pp.alloc((size_t)(n_patches + 1) * 4)) ||
            (rc = d_pb.alloc(std::max<size_t>(nb, 16))))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_pr.p, patch_row, (size_t)n_patches * 4));
        ISO_HIP_CHECK(copy_h2d(d_pc.p, patch_col, (size_t)n_patches * 4));
        ISO_HIP_CHECK(copy_h2d(d_pp.p, patch_ptr, (size_t)(n_patches + 1) * 4));
        if (nb) ISO_HIP_CHECK(copy_h2d(d_pb.p, patch_bytes, nb));
        hipLaunchKernelGGL(k_msa_patch, dim3((n_patches + 3) / 4), dim3(256), 0, 0, d_M, n_cols, d_pr.as<uint32_t>(), d_pc.as<uint32_t>(), d_pp.as<uint32_t>(),
                           d_pb.as<uint8_t>(), n_patches);
        ISO_HIP_CHECK(hipGetLastError());
    }
    pl->msa_tag.valid = false;          // (the correction leaves the matrix as it is, but one build serves one correction)
    return msa_correct_core(d_M, n_rows, n_cols, degree, out_packed, packed_cap, out_offsets, out_n_cand, out_class_totals, kernel_ms);
}

// the built matrix, for tests (rows as the reference's create_multialignment_matrix would give them)
extern "C" int isocon_msa_read_built(isocon_store *s, uint32_t n_rows, uint32_t n_cols, uint8_t *out_matrix)
{
    if (!s || !out_matrix) return ISOCON_E_ARG;
    ScratchPool *pl = &s->pool;
    if (!pl->msa_tag.valid || pl->msa_tag.serial != s->serial || pl->msa_tag.n_rows != n_rows || pl->msa_tag.n_cols != n_cols) return ISOCON_E_ARG;
    ISO_HIP_CHECK(copy_d2h(out_matrix, pl->slots[SLOT_MSA_IN].p, (size_t)n_rows * n_cols));
    return ISOCON_OK;
}

// ---- all partitions of a correction step in one set of launches (msa_batch.hpp) ------------------------------------------------------
namespace {

MsaBatch msa_batch_desc(ScratchPool *pl, uint32_t n_parts, uint32_t n_rows)
{
    MsaBatch B;
    B.part_of_row = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_PART].p);
    B.first_row = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_FIRST].p);
    B.Lm = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_LM].p);
    B.slot_base = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_SBASE].p);
    B.ncols = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_NCOLS].p);
    B.m_off = static_cast<const unsigned long long *>(pl->slots[SLOT_MSAB_MOFF].p);
    B.col_base = static_cast<const uint32_t *>(pl->slots[SLOT_MSAB_CBASE].p);
    B.n_parts = n_parts;
    B.n_rows = n_rows;
    return B;
}

}  // namespace

extern "C" int isocon_msa_build_ops_batch(isocon_store *s, uint32_t n_parts, const uint32_t *first_row, const uint32_t *row_ids, const uint32_t *ops,
                                          const uint64_t *ops_ptr, uint32_t *out_n_cols, uint32_t *out_col_slot, uint32_t *out_longest, uint32_t *out_wide,
                                          uint64_t wide_cap, uint64_t *n_wide, float *kernel_ms)
{
    if (!s || !first_row || !row_ids || !ops_ptr || !out_n_cols || !n_wide || n_parts == 0 || (wide_cap && !out_wide)) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (!s->acgt) { g_last_error = "the consensus correction needs a store over the alphabet ACGT"; return ISOCON_E_ALPHABET; }
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
        if (ops_ptr[first_row[p] + 1] != ops_ptr[first_row[p]]) { g_last_error = "the first row of a partition is its centre: it has no ops"; return ISOCON_E_ARG; }
        Lm[p] = (uint32_t)s->lens[row_ids[first_row[p]]];
        if ((uint64_t)slot_base[p] + Lm[p] + 1 > 0xffffffffull) { g_last_error = "too many insertion slots in one batch"; return ISOCON_E_UNSUPPORTED; }
        slot_base[p + 1] = slot_base[p] + Lm[p] + 1;
    }
    const uint64_t n_ops = ops_ptr[n_rows];
    if (ops_ptr[0] != 0 || (n_ops && !ops)) return ISOCON_E_ARG;
    const uint32_t n_slots = slot_base[n_parts];
    ScratchPool *pl = &s->pool;
    pl->msa_tag = MsaTag();
    pl->msab = MsaBatchHost();
    DevBuf d_rows(pl, SLOT_MSA_ROWS), d_ops(pl, SLOT_MSA_OPS), d_optr(pl, SLOT_MSA_OPTR), d_longest(pl, SLOT_MSA_LONGEST), d_width(pl, SLOT_MSA_WIDTH),
        d_cslot(pl, SLOT_MSA_CSLOT), d_tot(pl, SLOT_MSA_LTOT), d_wide(pl, SLOT_MSA_WIDE), d_M(pl, SLOT_MSA_IN), d_part(pl, SLOT_MSAB_PART), d_first(pl, SLOT_MSAB_FIRST),
        d_lm(pl, SLOT_MSAB_LM), d_sbase(pl, SLOT_MSAB_SBASE), d_ncols(pl, SLOT_MSAB_NCOLS), d_moff(pl, SLOT_MSAB_MOFF), d_cbase(pl, SLOT_MSAB_CBASE);
    int rc;
    if ((rc = d_rows.alloc((size_t)n_rows * 4)) || (rc = d_ops.alloc((size_t)std::max<uint64_t>(n_ops, 1) * 4)) || (rc = d_optr.alloc((size_t)(n_rows + 1) * 8)) ||
        (rc = d_longest.alloc((size_t)n_slots * 4)) || (rc = d_width.alloc((size_t)n_slots * 4)) || (rc = d_cslot.alloc((size_t)n_slots * 4)) || (rc = d_tot.alloc(32)) ||
        (rc = d_wide.alloc((size_t)std::max<uint64_t>(wide_cap, 1) * 32)) || (rc = d_part.alloc((size_t)n_rows * 4)) || (rc = d_first.alloc((size_t)(n_parts + 1) * 4)) ||
        (rc = d_lm.alloc((size_t)n_parts * 4)) || (rc = d_sbase.alloc((size_t)(n_parts + 1) * 4)) || (rc = d_ncols.alloc((size_t)n_parts * 4)) ||
        (rc = d_moff.alloc((size_t)(n_parts + 1) * 8)) || (rc = d_cbase.alloc((size_t)(n_parts + 1) * 4)))
        return rc;
    ISO_HIP_CHECK(copy_h2d(d_rows.p, row_ids, (size_t)n_rows * 4));
    if (n_ops) ISO_HIP_CHECK(copy_h2d(d_ops.p, ops, (size_t)n_ops * 4));
    ISO_HIP_CHECK(copy_h2d(d_optr.p, ops_ptr, (size_t)(n_rows + 1) * 8));
    ISO_HIP_CHECK(copy_h2d(d_part.p, part_of_row.data(), (size_t)n_rows * 4));
    ISO_HIP_CHECK(copy_h2d(d_first.p, first_row, (size_t)(n_parts + 1) * 4));
    ISO_HIP_CHECK(copy_h2d(d_lm.p, Lm.data(), (size_t)n_parts * 4));
    ISO_HIP_CHECK(copy_h2d(d_sbase.p, slot_base.data(), (size_t)(n_parts + 1) * 4));
    ISO_HIP_CHECK(hipMemsetAsync(d_longest.p, 0, (size_t)n_slots * 4, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, 32, 0));
    MsaBatch B = msa_batch_desc(pl, n_parts, n_rows);
    uint32_t *tot = d_tot.as<uint32_t>();          // [2] bad flag, [4..5] wide records (64 bit)
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_msab_ops_scan, dim3((n_rows + 255) / 256), dim3(256), 0, 0, s->dev, B, d_rows.as<uint32_t>(), d_ops.as<uint32_t>(), d_optr.as<unsigned long long>(),
                       d_longest.as<uint32_t>(), tot + 2);
    hipLaunchKernelGGL(k_msab_layout, dim3(n_parts), dim3(1024), 0, 0, B, d_longest.as<uint32_t>(), d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), d_ncols.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    uint32_t h_tot[4];
    ISO_HIP_CHECK(hipMemcpy(h_tot, d_tot.p, 16, hipMemcpyDeviceToHost));
    if (h_tot[2]) { g_last_error = "the ops of a row do not spell the centre and the member"; return ISOCON_E_ARG; }
    MsaBatchHost &H = pl->msab;
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
    if ((rc = d_M.alloc(std::max<size_t>(cells, 16)))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_moff.p, H.m_off.data(), (size_t)(n_parts + 1) * 8));
    ISO_HIP_CHECK(copy_h2d(d_cbase.p, H.col_base.data(), (size_t)(n_parts + 1) * 4));
    ISO_HIP_CHECK(hipMemsetAsync(d_M.p, '-', cells, 0));
    tm.start();
    hipLaunchKernelGGL(k_msab_fill, dim3((n_rows + 3) / 4), dim3(256), 0, 0, s->dev, B, d_rows.as<uint32_t>(), d_ops.as<uint32_t>(), d_optr.as<unsigned long long>(),
                       d_longest.as<uint32_t>(), d_width.as<uint32_t>(), d_cslot.as<uint32_t>(), d_M.as<uint8_t>(), d_wide.as<uint32_t>(), (unsigned long long)wide_cap,
                       reinterpret_cast<unsigned long long *>(tot + 4));
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    unsigned long long cnt = 0;
    ISO_HIP_CHECK(hipMemcpy(&cnt, tot + 4, 8, hipMemcpyDeviceToHost));
    *n_wide = cnt;
    if (cnt > wide_cap) return ISOCON_E_CAPACITY;
    if (cnt) ISO_HIP_CHECK(copy_d2h(out_wide, d_wide.p, (size_t)cnt * 32));
    if (out_col_slot) ISO_HIP_CHECK(copy_d2h(out_col_slot, d_cslot.p, (size_t)n_slots * 4));
    if (out_longest) ISO_HIP_CHECK(copy_d2h(out_longest, d_longest.p, (size_t)n_slots * 4));
    H.valid = true;
    H.serial = s->serial;
    H.n_parts = n_parts;
    H.n_rows = n_rows;
    return ISOCON_OK;
}

extern "C" int isocon_msa_correct_built_batch(isocon_store *s, uint32_t n_parts, uint32_t n_rows, const uint32_t *patch_row, const uint32_t *patch_col,
                                              const uint32_t *patch_ptr, const uint8_t *patch_bytes, uint32_t n_patches, const int32_t *degree,
                                              uint8_t *out_packed, uint64_t packed_cap, uint64_t *out_offsets, int32_t *out_n_cand, float *kernel_ms)
{
    if (!s || !degree || !out_offsets || !out_n_cand || (packed_cap && !out_packed) || n_parts == 0 || n_rows == 0 ||
        (n_patches && (!patch_row || !patch_col || !patch_ptr || !patch_bytes)))
        return ISOCON_E_ARG;
    ScratchPool *pl = &s->pool;
    MsaBatchHost &H = pl->msab;
    if (!H.valid || H.serial != s->serial || H.n_parts != n_parts || H.n_rows != n_rows) {
        g_last_error = "no batch of this shape was built for this store (isocon_msa_build_ops_batch comes first)";
        return ISOCON_E_ARG;
    }
    if (kernel_ms) *kernel_ms = 0.f;
    H.valid = false;
    MsaBatch B = msa_batch_desc(pl, n_parts, n_rows);
    uint8_t *d_M = static_cast<uint8_t *>(pl->slots[SLOT_MSA_IN].p);
    const size_t cells = (size_t)H.m_off[n_parts];
    const uint32_t n_colsum = H.col_base[n_parts];
    int rc;
    EventTimer tm;
    if (n_patches) {
        for (uint32_t i = 0; i < n_patches; ++i) {
            if (patch_row[i] >= n_rows || patch_ptr[i + 1] < patch_ptr[i]) { g_last_error = "patch outside the batch"; return ISOCON_E_ARG; }
            const uint32_t p = (uint32_t)(std::upper_bound(H.first_row.begin(), H.first_row.end(), patch_row[i]) - H.first_row.begin()) - 1;
            if ((uint64_t)patch_col[i] + (patch_ptr[i + 1] - patch_ptr[i]) > H.ncols[p]) { g_last_error = "patch outside its matrix"; return ISOCON_E_ARG; }
        }
        DevBuf d_pr(pl, SLOT_MSA_PROW), d_pc(pl, SLOT_MSA_PCOL), d_pp(pl, SLOT_MSA_PPTR), d_pb(pl, SLOT_MSA_PBYTES);
        const size_t nb = patch_ptr[n_patches];
        if ((rc = d_pr.alloc((size_t)n_patches * 4)) || (rc = d_pc.alloc((size_t)n_patches * 4)) || (rc = d_pp.alloc((size_t)(n_patches + 1) * 4)) ||
            (rc = d_pb.alloc(std::max<size_t>(nb, 16))))
            return rc;
        ISO_HIP_CHECK(copy_h2d(d_pr.p, patch_row, (size_t)n_patches * 4));
        ISO_HIP_CHECK(copy_h2d(d_pc.p, patch_col, (size_t)n_patches * 4));
        ISO_HIP_CHECK(copy_h2d(d_pp.p, patch_ptr, (size_t)(n_patches + 1) * 4));
        if (nb) ISO_HIP_CHECK(copy_h2d(d_pb.p, patch_bytes, nb));
        hipLaunchKernelGGL(k_msab_patch, dim3((n_patches + 3) / 4), dim3(256), 0, 0, d_M, B, d_pr.as<uint32_t>(), d_pc.as<uint32_t>(), d_pp.as<uint32_t>(), d_pb.as<uint8_t>(),
                           n_patches);
        ISO_HIP_CHECK(hipGetLastError());
    }
    // the column blocks of all partitions, and the same cut into chunks of MSAB_ROWS_PER_WG rows for the counting launch
    std::vector<uint32_t> cb_part, cb_col0, cbr;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const uint32_t nr = H.first_row[p + 1] - H.first_row[p];
        for (uint32_t c0 = 0; c0 < H.ncols[p]; c0 += 256) {
            cb_part.push_back(p); cb_col0.push_back(c0);
            for (uint32_t r0 = 0; r0 < nr; r0 += MSAB_ROWS_PER_WG) { cbr.push_back(p); cbr.push_back(c0); cbr.push_back(r0); }
        }
    }
    DevBuf d_out(pl, SLOT_MSA_OUT), d_deg(pl, SLOT_MSA_DEG), d_counts(pl, SLOT_MSA_COUNTS), d_maj(pl, SLOT_MSA_MAJ), d_flags(pl, SLOT_MSA_FLAGS), d_tot(pl, SLOT_MSA_TOT),
        d_ncand(pl, SLOT_MSA_NCAND), d_len(pl, SLOT_MSA_LEN), d_off(pl, SLOT_MSA_OFF), d_packed(pl, SLOT_MSA_PACKED), d_cbp(pl, SLOT_MSAB_CBP), d_cbc(pl, SLOT_MSAB_CBC), d_cbr(pl, SLOT_MSAB_CBR);
    if ((rc = d_out.alloc(std::max<size_t>(cells, 16))) || (rc = d_deg.alloc((size_t)n_rows * 4)) || (rc = d_counts.alloc((size_t)5 * std::max<uint32_t>(n_colsum, 1) * 4)) ||
        (rc = d_maj.alloc(std::max<uint32_t>(n_colsum, 1))) || (rc = d_flags.alloc(std::max<uint32_t>(n_colsum, 1))) || (rc = d_tot.alloc((size_t)24 * n_parts)) ||
        (rc = d_ncand.alloc((size_t)n_rows * 4)) || (rc = d_len.alloc((size_t)n_rows * 4)) || (rc = d_off.alloc((size_t)(n_rows + 1) * 8)) ||
        (rc = d_cbp.alloc(std::max<size_t>(cb_part.size(), 1) * 4)) || (rc = d_cbc.alloc(std::max<size_t>(cb_part.size(), 1) * 4)) ||
        (rc = d_cbr.alloc(std::max<size_t>(cbr.size(), 3) * 4)))
        return rc;
    ISO_HIP_CHECK(copy_h2d(d_deg.p, degree, (size_t)n_rows * 4));
    if (!cb_part.empty()) {
        ISO_HIP_CHECK(copy_h2d(d_cbp.p, cb_part.data(), cb_part.size() * 4));
        ISO_HIP_CHECK(copy_h2d(d_cbc.p, cb_col0.data(), cb_col0.size() * 4));
        if (!cbr.empty()) ISO_HIP_CHECK(copy_h2d(d_cbr.p, cbr.data(), cbr.size() * 4));
    }
    ISO_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, (size_t)24 * n_parts, 0));
    ISO_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, (size_t)5 * std::max<uint32_t>(n_colsum, 1) * 4, 0));
    tm.start();
    if (!cbr.empty())
        hipLaunchKernelGGL(k_msab_col_counts, dim3((unsigned)(cbr.size() / 3)), dim3(256), 0, 0, d_M, B, d_cbr.as<uint32_t>(), d_deg.as<int32_t>(), d_counts.as<int32_t>());
    if (!cb_part.empty())
        hipLaunchKernelGGL(k_msab_col_finish, dim3((unsigned)cb_part.size()), dim3(256), 0, 0, B, d_cbp.as<uint32_t>(), d_cbc.as<uint32_t>(),
                           d_counts.as<int32_t>(), d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>());
    hipLaunchKernelGGL(k_msab_row_correct, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_M, d_out.as<uint8_t>(), B, d_deg.as<int32_t>(), d_counts.as<int32_t>(),
                       d_maj.as<uint8_t>(), d_flags.as<uint8_t>(), d_tot.as<unsigned long long>(), d_ncand.as<int32_t>());
    hipLaunchKernelGGL(k_msab_row_lengths, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), B, d_len.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    ISO_HIP_CHECK(copy_d2h(out_n_cand, d_ncand.p, (size_t)n_rows * 4));
    std::vector<uint32_t> len(n_rows);
    ISO_HIP_CHECK(copy_d2h(len.data(), d_len.p, (size_t)n_rows * 4));
    out_offsets[0] = 0;
    for (uint32_t r = 0; r < n_rows; ++r) out_offsets[r + 1] = out_offsets[r] + len[r];
    const uint64_t total = out_offsets[n_rows];
    if (total > packed_cap) { H.valid = true; return ISOCON_E_CAPACITY; }          // (the built matrices are still there: call again with room)
    if ((rc = d_packed.alloc(total ? total : 16))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_off.p, out_offsets, (size_t)(n_rows + 1) * 8));
    tm.start();
    hipLaunchKernelGGL(k_msab_strip, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_out.as<uint8_t>(), B, d_off.as<uint64_t>(), d_packed.as<uint8_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (total) ISO_HIP_CHECK(copy_d2h(out_packed, d_packed.p, total));
    if (kernel_ms) *kernel_ms = tm.total;
    return ISOCON_OK;
}

