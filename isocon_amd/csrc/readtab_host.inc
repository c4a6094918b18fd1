// readtab_host.inc -- host side of the device read tables of the statistical test (included by isocon_hip.hip): isocon_readtab_create /
// _support / _set_qualities / _quality / _probability / _destroy / _device_bytes.  The tables live in the handle; the candidates' rows (needed by the build only), the queries and
// the answers pass through slots of the process' scratch pool.

struct isocon_readtab {
    uint64_t *d_row_ptr = nullptr, *d_blk_ptr = nullptr, *d_nob = nullptr, *d_diff = nullptr;
    uint32_t *d_pre = nullptr, *d_first = nullptr;
    uint8_t *d_read = nullptr;
    // only after isocon_readtab_set_qualities:
    uint64_t *d_rgap = nullptr, *d_qual_ptr = nullptr;
    uint32_t *d_rpre = nullptr, *d_rec_start = nullptr;
    uint8_t *d_qual = nullptr;
    bool has_qualities = false;
    uint64_t quality_bytes = 0;               // their share of device_bytes
    uint32_t n_rows = 0, n_tables = 0;
    uint64_t n_blk = 0;
    std::vector<uint32_t> first_row;          // host copies: what a query is checked against
    std::vector<int64_t> ref_len;             // candidate bases of every row of table k (-1: the table has no rows)
    uint64_t device_bytes = 0;
};

namespace {

template <class T>
int rt_alloc(isocon_readtab *h, T **p, size_t count)
{
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc((void **)p, bytes) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); g_last_error = "hipMalloc(read tables, " + std::to_string(bytes) + " B) failed"; return ISOCON_E_HIP; }
    h->device_bytes += bytes;
    return ISOCON_OK;
}

// appends n items to a byte image at the next multiple of 8 and returns their offset
template <class T>
size_t rt_pack(std::vector<uint8_t> &img, const T *src, size_t n)
{
    const size_t at = (img.size() + 7) & ~(size_t)7;
    img.resize(at + n * sizeof(T));
    if (n) memcpy(img.data() + at, src, n * sizeof(T));
    return at;
}

void rt_drop_qualities(isocon_readtab *h)
{
    void *bufs[] = {h->d_rgap, h->d_rpre, h->d_qual, h->d_qual_ptr, h->d_rec_start};
    for (void *p : bufs) if (p) (void)hipFree(p);
    h->d_rgap = h->d_qual_ptr = nullptr;
    h->d_rpre = h->d_rec_start = nullptr;
    h->d_qual = nullptr;
    h->device_bytes -= h->quality_bytes;
    h->quality_bytes = 0;
    h->has_qualities = false;
}

int readtab_create_impl(isocon_readtab *h, const uint8_t *ref_rows, const uint8_t *read_rows, const uint64_t *row_ptr, uint32_t n_rows, const uint32_t *first_row,
                        uint32_t n_tables, uint32_t *out_errors, float *kernel_ms)
{
    std::vector<uint64_t> blk_ptr((size_t)n_rows + 1, 0);
    for (uint32_t r = 0; r < n_rows; ++r) blk_ptr[r + 1] = blk_ptr[r] + (row_ptr[r + 1] - row_ptr[r] + 63) / 64;
    const uint64_t base = row_ptr[0], total = row_ptr[n_rows] - base, n_blk = blk_ptr[n_rows];
    std::vector<uint64_t> rel((size_t)n_rows + 1);
    for (uint32_t r = 0; r <= n_rows; ++r) rel[r] = row_ptr[r] - base;
    h->n_rows = n_rows;
    h->n_tables = n_tables;
    h->n_blk = n_blk;
    h->first_row.assign(first_row, first_row + n_tables + 1);
    int rc;
    if ((rc = rt_alloc(h, &h->d_row_ptr, (size_t)n_rows + 1)) || (rc = rt_alloc(h, &h->d_blk_ptr, (size_t)n_rows + 1)) || (rc = rt_alloc(h, &h->d_nob, n_blk)) ||
        (rc = rt_alloc(h, &h->d_diff, n_blk)) || (rc = rt_alloc(h, &h->d_pre, n_blk)) || (rc = rt_alloc(h, &h->d_first, (size_t)n_tables + 1)) ||
        (rc = rt_alloc(h, &h->d_read, total)))
        return rc;
    DevBuf d_ref(&g_scratch, SLOT_RT_REF), d_out(&g_scratch, SLOT_RT_OUT);
    if ((rc = d_ref.alloc(total)) || (rc = d_out.alloc(((size_t)n_rows * 4 + 1) * 4))) return rc;
    ISO_HIP_CHECK(copy_h2d(h->d_row_ptr, rel.data(), ((size_t)n_rows + 1) * 8));
    ISO_HIP_CHECK(copy_h2d(h->d_blk_ptr, blk_ptr.data(), ((size_t)n_rows + 1) * 8));
    ISO_HIP_CHECK(copy_h2d(h->d_first, first_row, ((size_t)n_tables + 1) * 4));
    if (total) {
        ISO_HIP_CHECK(copy_h2d(d_ref.p, ref_rows + base, total));
        ISO_HIP_CHECK(copy_h2d(h->d_read, read_rows + base, total));
    }
    uint32_t *d_bad = d_out.as<uint32_t>() + (size_t)n_rows * 4;
    ISO_HIP_CHECK(hipMemset(d_bad, 0, 4));
    EventTimer tm;
    if (n_rows) {
        tm.start();
        hipLaunchKernelGGL(k_rt_build, dim3((n_rows + 3) / 4), dim3(256), 0, 0, d_ref.as<uint8_t>(), h->d_read, h->d_row_ptr, h->d_blk_ptr, n_rows, h->d_nob, h->d_diff,
                           h->d_pre, d_out.as<uint32_t>(), d_bad);
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
    }
    if (kernel_ms) *kernel_ms = tm.total;
    std::vector<uint32_t> res((size_t)n_rows * 4 + 1);
    ISO_HIP_CHECK(copy_d2h(res.data(), d_out.p, res.size() * 4));
    if (res[(size_t)n_rows * 4]) { g_last_error = "isocon_readtab_create: a row holds a byte outside ACGT-"; return ISOCON_E_ARG; }
    h->ref_len.assign(n_tables, -1);
    for (uint32_t k = 0; k < n_tables; ++k)
        for (uint32_t r = first_row[k]; r < first_row[k + 1]; ++r) {
            const int64_t bases = res[(size_t)r * 4 + 3];
            if (h->ref_len[k] < 0) h->ref_len[k] = bases;
            else if (h->ref_len[k] != bases) {
                g_last_error = "isocon_readtab_create: the rows of table " + std::to_string(k) + " hold " + std::to_string(h->ref_len[k]) + " and " + std::to_string(bases) +
                               " candidate bases";
                return ISOCON_E_ARG;
            }
        }
    for (uint32_t r = 0; r < n_rows; ++r)
        for (int e = 0; e < 3; ++e) out_errors[(size_t)r * 3 + e] = res[(size_t)r * 4 + e];
    return ISOCON_OK;
}

}  // namespace

extern "C" void isocon_readtab_destroy(isocon_readtab *h)
{
    if (!h) return;
    void *bufs[] = {h->d_row_ptr, h->d_blk_ptr, h->d_nob, h->d_diff, h->d_pre, h->d_first, h->d_read};
    for (void *p : bufs) if (p) (void)hipFree(p);
    rt_drop_qualities(h);
    delete h;
}

extern "C" uint64_t isocon_readtab_device_bytes(const isocon_readtab *h) { return h ? h->device_bytes : 0; }

extern "C" int isocon_readtab_create(const uint8_t *ref_rows, const uint8_t *read_rows, const uint64_t *row_ptr, uint32_t n_rows, const uint32_t *first_row,
                                     uint32_t n_tables, isocon_readtab **out, uint32_t *out_errors, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!out) return ISOCON_E_ARG;
    *out = nullptr;
    if (!row_ptr || !first_row || (n_rows && !out_errors)) return ISOCON_E_ARG;
    if (first_row[0] != 0 || first_row[n_tables] != n_rows) { g_last_error = "isocon_readtab_create: first_row does not span the rows"; return ISOCON_E_ARG; }
    for (uint32_t k = 0; k < n_tables; ++k)
        if (first_row[k + 1] < first_row[k]) { g_last_error = "isocon_readtab_create: first_row descends"; return ISOCON_E_ARG; }
    for (uint32_t r = 0; r < n_rows; ++r)
        if (row_ptr[r + 1] < row_ptr[r] || row_ptr[r + 1] - row_ptr[r] > 0x7ffffff0ull) { g_last_error = "isocon_readtab_create: bad row_ptr at row " + std::to_string(r); return ISOCON_E_ARG; }
    if (row_ptr[n_rows] > row_ptr[0] && (!ref_rows || !read_rows)) return ISOCON_E_ARG;
    isocon_readtab *h = new isocon_readtab();
    const int rc = readtab_create_impl(h, ref_rows, read_rows, row_ptr, n_rows, first_row, n_tables, out_errors, kernel_ms);
    if (rc) { isocon_readtab_destroy(h); (void)hipGetLastError(); return rc; }
    *out = h;
    return ISOCON_OK;
}

namespace {

// What a query is answered with, and so how many slots its output range must hold.
enum RtAnswer { RT_ANSWER_BITS,          // ceil(rows / 64) words
                RT_ANSWER_CODES,         // variants x rows bytes
                RT_ANSWER_PROBS };       // rows doubles

// The queries of isocon_readtab_support / _quality / _probability (`what`: the entry's name) checked against the handle and uploaded as
// one image into d_in.  out_ptr: where query q's answer starts; it must hold what `answer` says.  Snippets are needed by the queries of
// kind 1, by all unless the answer is bits.  Coordinates in [-ref_len, 0) are wrapped as a Python index is.  tail / n_tail: doubles that
// travel at the end of the image (the probability entry's ratios and table), *d_tail: where they are on the device.
int rt_stage_queries(isocon_readtab *h, const char *what, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                     const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes, const uint64_t *out_ptr,
                     RtAnswer answer, DevBuf &d_in, RtQueries &Q, const double *tail = nullptr, size_t n_tail = 0, const double **d_tail = nullptr)
{
    const bool codes = answer != RT_ANSWER_BITS;
    const std::string name = what;
    if (!q_table || !q_kind || !var_ptr || !out_ptr) return ISOCON_E_ARG;
    const uint64_t n_var = var_ptr[n_queries], n_out = out_ptr[n_queries];
    if (n_var > ((uint64_t)1 << 40) || n_out > ((uint64_t)1 << 40)) return ISOCON_E_ARG;
    if (var_ptr[0] != 0 || out_ptr[0] != 0 || (n_var && (!var_pos || !var_u || !var_type))) return ISOCON_E_ARG;
    bool any_snippet = false;
    std::vector<uint32_t> pos((size_t)n_var);
    for (uint32_t q = 0; q < n_queries; ++q) {
        if (q_table[q] >= h->n_tables || q_kind[q] > 1 || var_ptr[q + 1] < var_ptr[q] || var_ptr[q + 1] > n_var || out_ptr[q + 1] < out_ptr[q] || out_ptr[q + 1] > n_out) {
            g_last_error = name + ": bad table, kind or offsets in query " + std::to_string(q);
            return ISOCON_E_ARG;
        }
        const uint32_t k = q_table[q], nr = h->first_row[k + 1] - h->first_row[k];
        const uint64_t need = answer == RT_ANSWER_CODES ? (var_ptr[q + 1] - var_ptr[q]) * nr : answer == RT_ANSWER_PROBS ? (uint64_t)nr : ((uint64_t)nr + 63) / 64;
        if (answer == RT_ANSWER_PROBS && var_ptr[q + 1] - var_ptr[q] > RT_P_MAX_VARIANTS) { g_last_error = name + ": too many variants in query " + std::to_string(q); return ISOCON_E_ARG; }
        if (out_ptr[q + 1] - out_ptr[q] < need) { g_last_error = name + ": the output range of query " + std::to_string(q) + " is too small"; return ISOCON_E_ARG; }
        const int64_t ref_len = h->ref_len[k];
        for (uint64_t v = var_ptr[q]; v < var_ptr[q + 1]; ++v) {
            int64_t i = var_pos[v];
            if (ref_len < 0) { pos[v] = 0; continue; }          // no rows: nothing is indexed
            if (i < -ref_len || i >= ref_len) {          // the per-read statement raises IndexError here
                g_last_error = name + ": coordinate " + std::to_string(i) + " of query " + std::to_string(q) + " outside a candidate of " + std::to_string(ref_len) + " bases";
                return ISOCON_E_ARG;
            }
            pos[v] = (uint32_t)(i < 0 ? i + ref_len : i);
        }
        any_snippet |= (codes || q_kind[q] == 1) && var_ptr[q + 1] > var_ptr[q];
    }
    std::vector<uint64_t> no_snippets;
    if (any_snippet) {
        if (!snip_ptr) return ISOCON_E_ARG;
        for (uint64_t v = 0; v < n_var; ++v)
            if (snip_ptr[v + 1] < snip_ptr[v]) { g_last_error = name + ": snip_ptr descends"; return ISOCON_E_ARG; }
        if (snip_ptr[n_var] > snip_ptr[0] && !snip_bytes) return ISOCON_E_ARG;
    } else {
        no_snippets.assign((size_t)n_var + 1, 0);
        snip_ptr = no_snippets.data();
    }
    const uint64_t snip_base = snip_ptr[0], snip_total = snip_ptr[n_var] - snip_base;
    std::vector<uint64_t> snip_rel((size_t)n_var + 1);
    for (uint64_t v = 0; v <= n_var; ++v) snip_rel[v] = snip_ptr[v] - snip_base;
    // one image of the queries, one copy
    std::vector<uint8_t> img;
    const size_t o_var_ptr = rt_pack(img, var_ptr, (size_t)n_queries + 1), o_snip_ptr = rt_pack(img, snip_rel.data(), snip_rel.size()),
                 o_out_ptr = rt_pack(img, out_ptr, (size_t)n_queries + 1), o_table = rt_pack(img, q_table, n_queries), o_pos = rt_pack(img, pos.data(), pos.size()),
                 o_u = rt_pack(img, var_u, (size_t)n_var), o_kind = rt_pack(img, q_kind, n_queries), o_type = rt_pack(img, var_type, (size_t)n_var),
                 o_snip = rt_pack(img, snip_total ? snip_bytes + snip_base : nullptr, (size_t)snip_total), o_tail = rt_pack(img, tail, n_tail);
    int rc;
    if ((rc = d_in.alloc(img.size()))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_in.p, img.data(), img.size()));
    const uint8_t *in = d_in.as<uint8_t>();
    Q = RtQueries{(const uint32_t *)(in + o_table), in + o_kind, (const uint64_t *)(in + o_var_ptr), (const uint32_t *)(in + o_pos), (const int32_t *)(in + o_u), in + o_type,
                  (const uint64_t *)(in + o_snip_ptr), in + o_snip, (const uint64_t *)(in + o_out_ptr), n_queries};
    if (d_tail) *d_tail = (const double *)(in + o_tail);
    return ISOCON_OK;
}

}  // namespace

extern "C" int isocon_readtab_support(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                                      const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                                      const uint64_t *bits_ptr, uint64_t *out_bits, uint32_t *out_count, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!h) return ISOCON_E_ARG;
    if (!n_queries) return ISOCON_OK;
    if (!bits_ptr || !out_count || (bits_ptr[n_queries] && !out_bits)) return ISOCON_E_ARG;
    DevBuf d_in(&g_scratch, SLOT_RT_IN), d_out(&g_scratch, SLOT_RT_OUT);
    RtQueries Q;
    int rc;
    if ((rc = rt_stage_queries(h, "isocon_readtab_support", n_queries, q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, bits_ptr, RT_ANSWER_BITS, d_in, Q)))
        return rc;
    const uint64_t n_words = bits_ptr[n_queries];
    const size_t out_bytes = (size_t)n_words * 8 + (size_t)n_queries * 4;
    if ((rc = d_out.alloc(out_bytes))) return rc;
    RtTables T{h->d_row_ptr, h->d_blk_ptr, h->d_nob, h->d_diff, h->d_pre, h->d_read, h->d_first};
    if (n_words) ISO_HIP_CHECK(hipMemset(d_out.p, 0, (size_t)n_words * 8));          // (words beyond a table's rows)
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_rt_support, dim3((n_queries + 3) / 4), dim3(256), 0, 0, T, Q, d_out.as<uint64_t>(), (uint32_t *)(d_out.as<uint8_t>() + (size_t)n_words * 8));
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    std::vector<uint8_t> res(out_bytes);
    ISO_HIP_CHECK(copy_d2h(res.data(), d_out.p, out_bytes));
    if (n_words) memcpy(out_bits, res.data(), (size_t)n_words * 8);
    memcpy(out_count, res.data() + (size_t)n_words * 8, (size_t)n_queries * 4);
    return ISOCON_OK;
}

extern "C" int isocon_readtab_set_qualities(isocon_readtab *h, const uint8_t *qual, const uint64_t *qual_ptr, const uint32_t *rec_start, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!h || !qual_ptr || (h->n_rows && !rec_start)) return ISOCON_E_ARG;
    const uint32_t n = h->n_rows;
    for (uint32_t r = 0; r < n; ++r)
        if (qual_ptr[r + 1] < qual_ptr[r] || qual_ptr[r + 1] - qual_ptr[r] > 0x7ffffff0ull) { g_last_error = "isocon_readtab_set_qualities: bad qual_ptr at row " + std::to_string(r); return ISOCON_E_ARG; }
    const uint64_t base = qual_ptr[0], total = qual_ptr[n] - base;
    if (total && !qual) return ISOCON_E_ARG;
    for (uint64_t x = 0; x < total; ++x)
        if (qual[base + x] > 93) { g_last_error = "isocon_readtab_set_qualities: a quality above 93"; return ISOCON_E_ARG; }
    rt_drop_qualities(h);          // a second call replaces the first
    std::vector<uint64_t> rel((size_t)n + 1);
    for (uint32_t r = 0; r <= n; ++r) rel[r] = qual_ptr[r] - base;
    const uint64_t before = h->device_bytes;
    int rc;
    if ((rc = rt_alloc(h, &h->d_rgap, h->n_blk)) || (rc = rt_alloc(h, &h->d_rpre, h->n_blk)) || (rc = rt_alloc(h, &h->d_qual, total)) ||
        (rc = rt_alloc(h, &h->d_qual_ptr, (size_t)n + 1)) || (rc = rt_alloc(h, &h->d_rec_start, n))) {
        h->quality_bytes = h->device_bytes - before;
        rt_drop_qualities(h);
        return rc;
    }
    h->quality_bytes = h->device_bytes - before;
    ISO_HIP_CHECK(copy_h2d(h->d_qual_ptr, rel.data(), ((size_t)n + 1) * 8));
    if (n) ISO_HIP_CHECK(copy_h2d(h->d_rec_start, rec_start, (size_t)n * 4));
    if (total) ISO_HIP_CHECK(copy_h2d(h->d_qual, qual + base, total));
    EventTimer tm;
    if (n) {
        tm.start();
        hipLaunchKernelGGL(k_rt_read_prefix, dim3((n + 3) / 4), dim3(256), 0, 0, h->d_read, h->d_row_ptr, h->d_blk_ptr, n, h->d_rgap, h->d_rpre);
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
    }
    if (kernel_ms) *kernel_ms = tm.total;
    h->has_qualities = true;
    return ISOCON_OK;
}

extern "C" int isocon_readtab_quality(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                                      const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                                      const uint64_t *code_ptr, uint8_t *out_codes, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!h) return ISOCON_E_ARG;
    if (!h->has_qualities) { g_last_error = "isocon_readtab_quality: the table set has no qualities (isocon_readtab_set_qualities)"; return ISOCON_E_ARG; }
    if (!n_queries) return ISOCON_OK;
    if (!code_ptr || (code_ptr[n_queries] && !out_codes)) return ISOCON_E_ARG;
    DevBuf d_in(&g_scratch, SLOT_RT_IN), d_out(&g_scratch, SLOT_RT_OUT);
    RtQueries Q;
    int rc;
    if ((rc = rt_stage_queries(h, "isocon_readtab_quality", n_queries, q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, code_ptr, RT_ANSWER_CODES, d_in, Q)))
        return rc;
    const uint64_t n_codes = code_ptr[n_queries];
    if (!n_codes) return ISOCON_OK;
    if ((rc = d_out.alloc((size_t)n_codes))) return rc;
    ISO_HIP_CHECK(hipMemset(d_out.p, 0, (size_t)n_codes));          // (bytes beyond variants x rows)
    RtTables T{h->d_row_ptr, h->d_blk_ptr, h->d_nob, h->d_diff, h->d_pre, h->d_read, h->d_first};
    RtQualities U{h->d_rgap, h->d_rpre, h->d_qual, h->d_qual_ptr, h->d_rec_start};
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_rt_quality, dim3((n_queries + 3) / 4), dim3(256), 0, 0, T, U, Q, d_out.as<uint8_t>());
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    ISO_HIP_CHECK(copy_d2h(out_codes, d_out.p, (size_t)n_codes));
    return ISOCON_OK;
}

extern "C" int isocon_readtab_probability(isocon_readtab *h, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr,
                                          const int32_t *var_pos, const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes,
                                          const double *q_ratios, const double *p_of_quality, const uint64_t *prob_ptr, double *out_prob, uint32_t *out_status,
                                          float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.f;
    if (!h) return ISOCON_E_ARG;
    if (!h->has_qualities) { g_last_error = "isocon_readtab_probability: the table set has no qualities (isocon_readtab_set_qualities)"; return ISOCON_E_ARG; }
    if (!n_queries) return ISOCON_OK;
    if (!q_ratios || !p_of_quality || !prob_ptr || !out_status || (prob_ptr[n_queries] && !out_prob)) return ISOCON_E_ARG;
    DevBuf d_in(&g_scratch, SLOT_RT_IN), d_out(&g_scratch, SLOT_RT_OUT);
    RtQueries Q;
    std::vector<double> tail((size_t)n_queries * 3 + 94);          // the queries' ratios, then the table
    memcpy(tail.data(), q_ratios, (size_t)n_queries * 3 * sizeof(double));
    memcpy(tail.data() + (size_t)n_queries * 3, p_of_quality, 94 * sizeof(double));
    const double *d_tail = nullptr;
    int rc;
    if ((rc = rt_stage_queries(h, "isocon_readtab_probability", n_queries, q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, prob_ptr, RT_ANSWER_PROBS,
                               d_in, Q, tail.data(), tail.size(), &d_tail)))
        return rc;
    const uint64_t n_prob = prob_ptr[n_queries];
    const size_t out_bytes = (size_t)n_prob * 8 + (size_t)n_queries * 4;
    if ((rc = d_out.alloc(out_bytes))) return rc;
    if (n_prob) ISO_HIP_CHECK(hipMemset(d_out.p, 0, (size_t)n_prob * 8));          // (slots beyond a table's rows)
    RtTables T{h->d_row_ptr, h->d_blk_ptr, h->d_nob, h->d_diff, h->d_pre, h->d_read, h->d_first};
    RtQualities U{h->d_rgap, h->d_rpre, h->d_qual, h->d_qual_ptr, h->d_rec_start};
    uint32_t *d_status = (uint32_t *)(d_out.as<uint8_t>() + (size_t)n_prob * 8);
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_rt_probability, dim3((n_queries + 3) / 4), dim3(256), 0, 0, T, U, Q, d_tail, d_tail + (size_t)n_queries * 3, d_out.as<double>(), d_status);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    if (n_prob) ISO_HIP_CHECK(copy_d2h(out_prob, d_out.p, (size_t)n_prob * 8));
    ISO_HIP_CHECK(copy_d2h(out_status, d_status, (size_t)n_queries * 4));
    return ISOCON_OK;
}
