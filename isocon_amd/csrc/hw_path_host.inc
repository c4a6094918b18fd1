// hw_path_host.inc -- host side of isocon_hw_path_pairs (included by isocon_hip.hip after nw_path_host.inc): the rows through the
// implementation of isocon_hw_pairs_wide (banded kernels where the band fits), then the path of every hit as the global alignment of
// the query against its located window t[start..end], through the windowed instance of nw_path.hpp and the driver of nw_path_host.inc.

extern "C" int isocon_hw_path_pairs(isocon_store *s, const uint32_t *q, const uint32_t *t, const int32_t *k, uint64_t n_pairs,
                                    int32_t *out, uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *needed, float *kernel_ms)
{
    int rc;
    if (path_prologue(s, n_pairs, {q, t, k, out}, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms, &rc)) return rc;
    HostClock clk;
    // ---- rows: distance, location and terminal insertion runs; the argument checks are that entry's ----
    float ms_rows = 0.f;
    if ((rc = isocon_hw_pairs_wide(s, q, t, k, n_pairs, out, &ms_rows))) return rc;
    clk.lap("hw path: rows");
    // ---- the hits and their windows, then what both path entries share ----
    const std::vector<int32_t> &lens = s->lens;
    NwpHits H;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const int32_t *o = out + p * 5;
        if (o[0] < 0) continue;
        if (o[1] < 0 || o[2] < o[1] || o[2] >= lens[t[p]]) {
            g_last_error = "isocon_hw_path_pairs: internal status (location) for pair " + std::to_string(p);
            return ISOCON_E_HIP;
        }
        H.pair.push_back(p); H.q.push_back(q[p]); H.t.push_back(t[p]); H.ed.push_back(o[0]);
        H.start.push_back(o[1]); H.cols.push_back(o[2] - o[1] + 1);
    }
    if (kernel_ms) *kernel_ms = ms_rows;
    return nwp_paths(s, "isocon_hw_path_pairs", "hw path", H, n_pairs, [](uint64_t) -> uint64_t { return 0; }, out_ops, out_ops_ptr, ops_cap, needed, kernel_ms,
                     clk);
}
