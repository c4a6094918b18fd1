// edgevar_host.inc -- host side of the edge variants of the statistical test (included by isocon_hip.hip): isocon_edge_variants.  Independent
// of a store: the candidates' bytes, the edges and their ops are uploaded per call as one image; the answers come back through slots of the
// process' scratch pool.  Two launches (edgevar.hpp) with the prefix sum over the snippet lengths made here in between.

extern "C" int isocon_edge_variants(const uint8_t *seqs, const uint64_t *seq_ptr, uint32_t n_seqs, uint32_t n_edges, const uint32_t *edge_t, const uint32_t *edge_c,
                                    const uint32_t *ops, const uint64_t *ops_ptr, const uint64_t *rec_ptr, uint8_t *out_flipped, uint32_t *out_n_var, uint8_t *out_bad,
                                    int32_t *out_recs, uint64_t *out_snip_ptr, uint8_t *out_snip_c, uint8_t *out_snip_t, uint64_t snip_cap, uint64_t *n_snip_needed,
                                    float *kernel_ms)
{
    const std::string name = "isocon_edge_variants";
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_snip_needed) *n_snip_needed = 0;
    if (!n_edges) return ISOCON_OK;
    if (!seq_ptr || !edge_t || !edge_c || !ops_ptr || !rec_ptr || !out_flipped || !out_n_var || !out_bad || !out_snip_ptr) return ISOCON_E_ARG;
    for (uint32_t s = 0; s < n_seqs; ++s)
        if (seq_ptr[s + 1] < seq_ptr[s] || seq_ptr[s + 1] - seq_ptr[s] > ((uint64_t)1 << 30)) { g_last_error = name + ": bad seq_ptr at sequence " + std::to_string(s); return ISOCON_E_ARG; }
    const uint64_t seq_base = n_seqs ? seq_ptr[0] : 0, seq_total = n_seqs ? seq_ptr[n_seqs] - seq_base : 0;
    if (seq_total && !seqs) return ISOCON_E_ARG;
    const uint64_t n_lists = 2 * (uint64_t)n_edges;
    for (uint32_t e = 0; e < n_edges; ++e) {
        if (edge_t[e] >= n_seqs || edge_c[e] >= n_seqs) { g_last_error = name + ": sequence id out of range in edge " + std::to_string(e); return ISOCON_E_ARG; }
        if (seq_ptr[edge_t[e] + 1] == seq_ptr[edge_t[e]] || seq_ptr[edge_c[e] + 1] == seq_ptr[edge_c[e]]) { g_last_error = name + ": empty sequence in edge " + std::to_string(e); return ISOCON_E_ARG; }
        if (ops_ptr[2 * (uint64_t)e + 1] < ops_ptr[2 * (uint64_t)e] || ops_ptr[2 * (uint64_t)e + 2] < ops_ptr[2 * (uint64_t)e + 1]) { g_last_error = name + ": ops_ptr descends in edge " + std::to_string(e); return ISOCON_E_ARG; }
        if (rec_ptr[e + 1] < rec_ptr[e]) { g_last_error = name + ": rec_ptr descends in edge " + std::to_string(e); return ISOCON_E_ARG; }
    }
    const uint64_t ops_base = ops_ptr[0], n_ops = ops_ptr[n_lists] - ops_base, rec_base = rec_ptr[0], n_slots = rec_ptr[n_edges] - rec_base;
    if (n_ops > ((uint64_t)1 << 32) || n_slots > ((uint64_t)1 << 32)) return ISOCON_E_ARG;
    if ((n_ops && !ops) || (n_slots && !out_recs)) return ISOCON_E_ARG;
    static const struct Acgt { bool ok[256] = {}; Acgt() { ok['A'] = ok['C'] = ok['G'] = ok['T'] = true; } } acgt;
    for (uint64_t x = 0; x < seq_total; ++x)
        if (!acgt.ok[seqs[seq_base + x]]) { g_last_error = name + ": a sequence holds a byte outside ACGT"; return ISOCON_E_ALPHABET; }
    // one image of the inputs, one copy
    std::vector<uint64_t> seq_rel((size_t)n_seqs + 1), ops_rel((size_t)n_lists + 1), rec_rel((size_t)n_edges + 1);
    for (uint32_t s = 0; s <= n_seqs; ++s) seq_rel[s] = seq_ptr[s] - seq_base;
    for (uint64_t l = 0; l <= n_lists; ++l) ops_rel[l] = ops_ptr[l] - ops_base;
    for (uint32_t e = 0; e <= n_edges; ++e) rec_rel[e] = rec_ptr[e] - rec_base;
    std::vector<uint8_t> img;
    const size_t o_seq_ptr = rt_pack(img, seq_rel.data(), seq_rel.size()), o_ops_ptr = rt_pack(img, ops_rel.data(), ops_rel.size()), o_rec_ptr = rt_pack(img, rec_rel.data(), rec_rel.size()),
                 o_et = rt_pack(img, edge_t, n_edges), o_ec = rt_pack(img, edge_c, n_edges), o_ops = rt_pack(img, n_ops ? ops + ops_base : nullptr, (size_t)n_ops),
                 o_seqs = rt_pack(img, seq_total ? seqs + seq_base : nullptr, (size_t)seq_total);
    // the answers: records, per-op prefix sums, counts and flags; then the snippet offsets and bytes
    const size_t a_recs = 0, a_pcol = a_recs + (size_t)n_slots * 32, a_pt = a_pcol + (size_t)n_ops * 4, a_pc = a_pt + (size_t)n_ops * 4, a_nvar = a_pc + (size_t)n_ops * 4,
                 a_flip = a_nvar + (size_t)n_edges * 4, a_bad = a_flip + n_edges, a_end = a_bad + n_edges;
    DevBuf d_in(&g_scratch, SLOT_EV_IN), d_out(&g_scratch, SLOT_EV_OUT), d_snip(&g_scratch, SLOT_EV_SNIP);
    int rc;
    if ((rc = d_in.alloc(img.size())) || (rc = d_out.alloc(a_end))) return rc;
    ISO_HIP_CHECK(copy_h2d(d_in.p, img.data(), img.size()));
    const uint8_t *in = d_in.as<uint8_t>();
    uint8_t *out = d_out.as<uint8_t>();
    const EvEdges E{in + o_seqs, (const uint64_t *)(in + o_seq_ptr), (const uint32_t *)(in + o_et), (const uint32_t *)(in + o_ec), (const uint32_t *)(in + o_ops),
                    (const uint64_t *)(in + o_ops_ptr), (const uint64_t *)(in + o_rec_ptr), n_edges};
    EventTimer tm;
    tm.start();
    hipLaunchKernelGGL(k_ev_records, dim3((n_edges + 3) / 4), dim3(256), 0, 0, E, out + a_flip, (uint32_t *)(out + a_nvar), out + a_bad, (int32_t *)(out + a_recs),
                       (uint32_t *)(out + a_pcol), (uint32_t *)(out + a_pt), (uint32_t *)(out + a_pc));
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    std::vector<uint8_t> tail(a_end - a_nvar);
    ISO_HIP_CHECK(copy_d2h(tail.data(), out + a_nvar, tail.size()));
    memcpy(out_n_var, tail.data(), (size_t)n_edges * 4);
    memcpy(out_flipped, tail.data() + (a_flip - a_nvar), n_edges);
    memcpy(out_bad, tail.data() + (a_bad - a_nvar), n_edges);
    for (uint32_t e = 0; e < n_edges; ++e)
        if (out_n_var[e] > rec_rel[e + 1] - rec_rel[e]) {
            g_last_error = name + ": edge " + std::to_string(e) + " has " + std::to_string(out_n_var[e]) + " variants, its capacity is " + std::to_string(rec_rel[e + 1] - rec_rel[e]);
            return ISOCON_E_ARG;
        }
    std::vector<int32_t> recs((size_t)n_slots * 8);
    if (n_slots) ISO_HIP_CHECK(copy_d2h(recs.data(), out + a_recs, recs.size() * 4));
    std::vector<uint64_t> snip_ptr((size_t)n_slots + 1, 0);
    for (uint32_t e = 0; e < n_edges; ++e) {
        for (uint64_t k = 0; k < rec_rel[e + 1] - rec_rel[e]; ++k) {
            const uint64_t s = rec_rel[e] + k;
            if (k >= out_n_var[e]) for (int f = 0; f < 8; ++f) recs[s * 8 + f] = 0;          // (slots beyond an edge's variants come back 0)
            snip_ptr[s + 1] = snip_ptr[s] + (uint64_t)recs[s * 8 + 6];
        }
    }
    if (n_slots) memcpy(out_recs, recs.data(), recs.size() * 4);
    memcpy(out_snip_ptr, snip_ptr.data(), snip_ptr.size() * 8);
    const uint64_t snip_total = snip_ptr[n_slots];
    if (n_snip_needed) *n_snip_needed = snip_total;
    if (!snip_total) return ISOCON_OK;
    if (snip_total > snip_cap) { g_last_error = name + ": the snippets need " + std::to_string(snip_total) + " bytes each way"; return ISOCON_E_CAPACITY; }
    if (!out_snip_c || !out_snip_t) return ISOCON_E_ARG;
    const size_t s_ptr = 0, s_c = ((size_t)n_slots + 1) * 8, s_t = s_c + (size_t)snip_total;
    if ((rc = d_snip.alloc(s_t + (size_t)snip_total))) return rc;
    uint8_t *sn = d_snip.as<uint8_t>();
    ISO_HIP_CHECK(copy_h2d(sn + s_ptr, snip_ptr.data(), snip_ptr.size() * 8));
    tm.start();
    hipLaunchKernelGGL(k_ev_snippets, dim3((n_edges + 3) / 4), dim3(256), 0, 0, E, out + a_flip, (const uint32_t *)(out + a_nvar), (const int32_t *)(out + a_recs),
                       (const uint32_t *)(out + a_pcol), (const uint32_t *)(out + a_pt), (const uint32_t *)(out + a_pc), (const uint64_t *)(sn + s_ptr), sn + s_c, sn + s_t);
    ISO_HIP_CHECK(hipGetLastError());
    tm.stop();
    if (kernel_ms) *kernel_ms = tm.total;
    ISO_HIP_CHECK(copy_d2h(out_snip_c, sn + s_c, (size_t)snip_total));
    ISO_HIP_CHECK(copy_d2h(out_snip_t, sn + s_t, (size_t)snip_total));
    return ISOCON_OK;
}
