// sg_host.inc -- host side of isocon_sg_trace_batch (included by isocon_hip.hip).
//
// Pairs are grouped by strip height R (64*R >= query length) and processed in batches that fit the trace scratch
// budget; per batch: forward kernels (one per R group), the walk kernel, a compaction kernel, one D2H of ops+res.

namespace {

static const int kSgR = 8;   // strip height of the forward kernel (rows per lane and pass)

template <int DPL>
void launch_sg_band(bool general, const DevStore &S, SgPair *d_pairs, const SgParams &prm, uint8_t *d_trace, int32_t *d_end, unsigned n, uint32_t *d_again)
{
    const bool ext0 = prm.ext == 0;
    if (!general && ext0) hipLaunchKernelGGL((k_sg_band<true, true, DPL>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_end, d_again);
    else if (!general) hipLaunchKernelGGL((k_sg_band<true, false, DPL>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_end, d_again);
    else if (ext0) hipLaunchKernelGGL((k_sg_band<false, true, DPL>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_end, d_again);
    else hipLaunchKernelGGL((k_sg_band<false, false, DPL>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_end, d_again);
}

void launch_sg_forward_R(bool general, const DevStore &S, const SgPair *d_pairs, const SgParams &prm, uint8_t *d_trace,
                         int2 *d_bound, int32_t *d_end, unsigned n)
{
    const bool ext0 = prm.ext == 0;
    if (!general && ext0) hipLaunchKernelGGL((k_sg_forward<kSgR, true, true>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_bound, d_end);
    else if (!general) hipLaunchKernelGGL((k_sg_forward<kSgR, true, false>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_bound, d_end);
    else if (ext0) hipLaunchKernelGGL((k_sg_forward<kSgR, false, true>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_bound, d_end);
    else hipLaunchKernelGGL((k_sg_forward<kSgR, false, false>), dim3(n), dim3(64), 0, 0, S, d_pairs, prm, d_trace, d_bound, d_end);
}

}  // namespace

namespace {
thread_local double g_sg_stats[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int sg_batch_impl(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t match,
                  const int8_t *mismatch_per_pair, int32_t open, int32_t ext, int32_t tie_policy,
                  uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *n_ops_needed,
                  int32_t *out_res, float *kernel_ms,
                  uint8_t *out_aln_a, uint8_t *out_aln_b, uint64_t *out_aln_ptr, uint64_t aln_cap, uint64_t *n_aln_needed,
                  const int32_t *ed_upper)
{
    if (s && !s->acgt) {          // parasail scores with a matrix over "ACGT" (SWM:65): its behaviour on other symbols is unpinned (SURVEY A6)
        g_last_error = "alignments need a store over the alphabet ACGT (this one holds other symbols)";
        return ISOCON_E_ALPHABET;
    }
    const bool want_strings = out_aln_ptr != nullptr;
    // gapped strings stay in their batch's download buffers; every pair remembers where (copied once, at the end)
    struct AlnRef { uint32_t batch; uint64_t off; uint64_t len; };
    std::vector<AlnRef> aln_ref;
    std::vector<std::unique_ptr<uint8_t[]>> batch_a, batch_b;      // (new[] without value-initialisation: 2 x 130 MB per C3 batch)
    if (want_strings) aln_ref.assign(n_pairs, AlnRef{0, 0, 0});
    bool strings_direct = false;     // the strings already lie in the caller's buffers (single-batch path)
    bool ops_direct = false;         // the ops already lie in the caller's buffer, out_ops_ptr is final (single-batch path)
    if (!s || !out_ops_ptr || (n_pairs && (!a || !b || !mismatch_per_pair || !out_res)) || (ops_cap && !out_ops)) return ISOCON_E_ARG;
    if (match <= 0 || open < 0 || ext < 0 || tie_policy < 0 || tie_policy > 31) return ISOCON_E_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    for (double &x : g_sg_stats) x = 0;
    const uint32_t n = s->dev.n;
    const std::vector<int32_t> &lens = s->lens;
    // the fast kernels implement policy 0 cell rules; end-cell bits are handled in every kernel
    const bool general = (tie_policy & (SG_POL_E_BEFORE_F | SG_POL_OPEN_ON_TIE | SG_POL_GAP_FIRST)) != 0;

    HostClock hc;
    std::vector<int> Rof(n_pairs, 0);
    std::vector<uint64_t> order;
    // run-length ops stay in their batch's download buffer; a pair remembers where (the 50 000 pairs of a C3 step: no vector per pair)
    struct OpsRef { uint32_t batch; uint32_t cnt; uint64_t off; };
    std::vector<OpsRef> ops_ref(n_pairs, OpsRef{0, 0, 0});
    std::vector<std::vector<uint32_t>> batch_ops(1);          // batch 0: the ops of degenerate pairs (an empty sequence)
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (a[p] >= n || b[p] >= n) return ISOCON_E_ARG;
        if (mismatch_per_pair[p] > 0) return ISOCON_E_ARG;
        const int32_t m = lens[a[p]], nn = lens[b[p]];
        if (m == 0 || nn == 0) {   // everything is an end gap (oracle: orc_sg_trace degenerate branch)
            ops_ref[p].off = batch_ops[0].size();
            if (m > 0) batch_ops[0].push_back(((uint32_t)m << 4) | 2u);
            if (nn > 0) batch_ops[0].push_back(((uint32_t)nn << 4) | 3u);
            ops_ref[p].cnt = (uint32_t)(batch_ops[0].size() - ops_ref[p].off);
            if (want_strings) {   // the non-empty sequence against gaps; decoded from nothing but its length is not possible
                g_last_error = "isocon_sg_strings_batch: empty sequence";
                return ISOCON_E_UNSUPPORTED;
            }
            int32_t *o = out_res + p * 6;
            o[0] = 0; o[1] = m - 1; o[2] = nn - 1; o[3] = 0; o[4] = 0; o[5] = m + nn;
            continue;
        }
        Rof[p] = kSgR;
        order.push_back(p);
    }
    // Band from the caller's edit-distance bound (SW_alignment_module hands the exact distance of every pair down).
    // An alignment that reaches a diagonal more than X outside the corner-to-corner corridor [min(0,D), max(0,D)],
    // D = n - m, can pair at most min(m,n) - X - 1 bases, so it scores <= match * (min(m,n) - X - 1); the edit script
    // behind the bound scores >= match * max(m,n) - (match + Q) * ed, Q = max(mismatch penalty, open + ext).  With
    // X >= (match + Q) * ed / match - |D| every optimal alignment -- and every tie among them -- lies inside the band,
    // and cells inside it whose best predecessors would lie outside are not on any optimal path: the banded result is
    // the full-matrix result.  The bound is not trusted: a pair is accepted only if its banded score exceeds
    // match * (min(m,n) - X - 1) (then nothing outside the band can reach it); otherwise it is aligned again in full.
    std::vector<int32_t> Xof(n_pairs, -1);
    if (ed_upper) {
        for (uint64_t p : order) {
            if (ed_upper[p] < 0) continue;
            const int64_t m = lens[a[p]], nn = lens[b[p]], D = nn - m, aD = D < 0 ? -D : D;
            const int64_t Q = std::max<int64_t>(-(int64_t)mismatch_per_pair[p], (int64_t)open + ext);
            int64_t X = ((int64_t)(match + Q) * ed_upper[p] + match - 1) / match - aD + 1;
            if (X < 1) X = 1;
            if (aD + 2 * X + 64 < std::min(m, nn)) Xof[p] = (int32_t)X;      // else the band is no smaller than the matrix
        }
    }
    hc.lap("sg: degenerate pairs, bands");
    std::vector<uint64_t> redo;      // pairs whose banded result could not be certified
    // A pair whose bound asks for 129 .. 256 diagonals first runs on the 128 diagonals around its corridor if that band keeps at least
    // SG_TRY_NARROW_PCT % of the half-width: the bound prices every edit as the dearest kind (match + Q), a read pair's mix of
    // substitutions and indels needs ~ 75-85 % of it (C3: 14 172 of 21 447 such pairs qualify, 1 is not certified), and two diagonals
    // per lane cost half of four.  The certificate is the same one, evaluated for the band that was run (k_sg_recheck, on the device,
    // between the forward kernels and the walks); a pair that fails it is run again in the band of its bound within the same batch.
    std::vector<int32_t> Xtry(n_pairs, -1);
    const bool no_try = variant("sw_no_narrow_try") || variant("sw_band256") || variant("sw_strips");
    int64_t SG_TRY_NARROW_PCT = 85;
    if (const char *e = variant_value("sw_narrow_try_pct")) SG_TRY_NARROW_PCT = std::max(1, atoi(e));      // tests: tries that fail
    if (ed_upper && !no_try) {
        for (uint64_t p : order) {
            if (Xof[p] < 0) continue;
            const int64_t D = (int64_t)lens[b[p]] - lens[a[p]], aD = D < 0 ? -D : D;
            const int64_t diags = aD + 2 * (int64_t)Xof[p] + 1;
            if (diags <= SG_BAND_DIAGS_NARROW || diags > SG_BAND_DIAGS) continue;
            const int64_t xn = (SG_BAND_DIAGS_NARROW - 1 - aD) / 2;
            if (xn >= 1 && xn * 100 >= SG_TRY_NARROW_PCT * Xof[p]) Xtry[p] = (int32_t)xn;
        }
    }
    // certified bands of at most 256 diagonals run with the diagonals on the lanes (k_sg_band), everything else in strips
    const bool no_diag_kernel = variant("sw_strips");
    const bool no_narrow = variant("sw_band256");          // every certified band on four diagonals per lane (A/B runs)
    // 0: strips; 1: the band's diagonals on the lanes, four per lane (<= 256 diagonals); 2: two per lane (<= 128: half the cells and trace)
    auto diag_mode = [&](uint64_t p, bool banded) -> int {
        if (!banded || Xof[p] < 0 || no_diag_kernel) return 0;
        const int64_t D = (int64_t)lens[b[p]] - lens[a[p]], aD = D < 0 ? -D : D;
        const int64_t diags = aD + 2 * (int64_t)Xof[p] + 1;
        if (diags <= SG_BAND_DIAGS_NARROW && !no_narrow) return 2;
        return diags <= SG_BAND_DIAGS ? 1 : 0;
    };
    auto pair_steps = [&](uint64_t p, bool banded) -> uint64_t {
        const int64_t m = lens[a[p]], nn = lens[b[p]];
        if (!banded || Xof[p] < 0) return (uint64_t)nn + 63;
        const int64_t D = nn - m;
        const int64_t width = 64 * kSgR + ((D > 0 ? D : 0) + Xof[p]) - ((D < 0 ? D : 0) - Xof[p]) + 2 + 64;     // rows + band + start alignment
        return (uint64_t)std::min<int64_t>(nn, width) + 63;
    };
    size_t free_b = 0, total_b = 0;
    ISO_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = std::min<uint64_t>((uint64_t)free_b / 2, (uint64_t)24 << 30);
    EventTimer tm, tm_compact, tm_expand;      // tm: forward kernels, then (behind its mark) the walks
    SgParams prm{match, open, ext, tie_policy};

  for (int round = 0; round < 2; ++round) {
    const bool banded = round == 0;
    if (round == 1) {
        if (redo.empty()) break;
        order.swap(redo);
    }
    // longest first: the few big alignments do not end up alone at the tail of a launch.  Descending cost, ties to the lower index: two
    // stable counting passes over 22-bit keys (a comparison sort of the 50 000 C3 pairs took 2.6 ms of a 19 ms call; costs above the cap --
    // 4 M steps -- count as equal: the order is a schedule, not a result)
    {
        const size_t no = order.size();
        if (round == 1) std::sort(order.begin(), order.end());          // (round 0: already ascending)
        constexpr uint32_t CAP = (1u << 22) - 1;
        std::vector<uint32_t> key(no), key2(no);
        std::vector<uint64_t> order2(no);
        for (size_t i = 0; i < no; ++i) {
            const uint64_t x = order[i];
            const uint64_t npx = ((uint64_t)lens[a[x]] + 64 * kSgR - 1) / (64 * kSgR);
            const int dmx = banded && Xtry[x] >= 0 ? 2 : diag_mode(x, banded);
            const uint64_t cx = dmx ? ((uint64_t)lens[a[x]] + lens[b[x]]) / (dmx == 2 ? 8 : 4) : npx * pair_steps(x, banded);
            key[i] = CAP - (uint32_t)std::min<uint64_t>(cx, CAP);
        }
        for (int pass = 0; pass < 2; ++pass) {
            const int shift = 11 * pass;
            std::vector<uint32_t> start(2049, 0);
            for (size_t i = 0; i < no; ++i) ++start[((key[i] >> shift) & 2047u) + 1];
            for (int d = 0; d < 2048; ++d) start[d + 1] += start[d];
            for (size_t i = 0; i < no; ++i) {
                const uint32_t at = start[(key[i] >> shift) & 2047u]++;
                order2[at] = order[i]; key2[at] = key[i];
            }
            order.swap(order2); key.swap(key2);
        }
    }

    hc.lap("sg: sort by cost");
    size_t pos = 0;
    while (pos < order.size()) {
        // assemble a batch.  (hp is the host's copy of the records as UPLOADED: a pair whose narrow try fails is run again inside k_sg_band,
        // which rewrites mode / dlo / dhi of its DEVICE record for the walk -- after the launch only d_pairs is authoritative)
        std::vector<SgPair> hp;
        std::vector<int32_t> hR;
        uint64_t tbytes = 0, oslots = 0, bslots = 0, n_diag = 0, n_diag2 = 0, n_try = 0;
        size_t end = pos;
        while (end < order.size() && hp.size() < 65536) {
            const uint64_t p = order[end];
            const int32_t m = lens[a[p]], nn = lens[b[p]];
            const uint64_t npass = ((uint64_t)m + 64 * kSgR - 1) / (64 * kSgR);
            const uint64_t st = pair_steps(p, banded);
            const int dm = diag_mode(p, banded);
            const bool tried = banded && Xtry[p] >= 0;          // (dm == 1: the trace region is sized for the band of the bound)
            // (k_sg_band: dwords of 8 / 4 steps per lane, in tiles of 16 per lane)
            const uint64_t tb = dm ? ((((uint64_t)m + nn + 2) / (dm == 2 ? 8 : 4) + 1 + SG_TILE_DWORDS - 1) / SG_TILE_DWORDS) * SG_TILE_DWORDS * 256
                                   : npass * st * 32 * (uint64_t)kSgR;
            if (!hp.empty() && tbytes + tb > budget) break;
            SgPair q;
            q.a = a[p]; q.b = b[p]; q.mismatch = mismatch_per_pair[p];
            q.steps = (int32_t)st;
            q.mode = tried ? 2 : dm; q.retry_x = tried ? Xof[p] : 0;
            n_diag += dm ? 1 : 0;
            n_diag2 += q.mode == 2 ? 1 : 0;
            n_try += tried ? 1 : 0;
            if (banded && Xof[p] >= 0) {
                const int32_t D = nn - m, xr = tried ? Xtry[p] : Xof[p];
                q.dlo = (D < 0 ? D : 0) - xr;
                q.dhi = (D > 0 ? D : 0) + xr;
            } else { q.dlo = -m - 1; q.dhi = nn + 1; }
            q.trace_off = tbytes; q.ops_off = oslots; q.bound_off = bslots;
            tbytes += (tb + 255) & ~(uint64_t)255;
            oslots += (uint64_t)m + nn + 2;
            bslots += (uint64_t)nn;
            hp.push_back(q);
            hR.push_back(Rof[p]);
            ++end;
        }
        if (tbytes > free_b - (free_b >> 3)) { g_last_error = "isocon_sg_trace_batch: trace scratch does not fit device memory"; return ISOCON_E_HIP; }
        const size_t nb = hp.size();
        ScratchPool *pl = &s->pool;
        DevBuf d_pairs(pl, SLOT_SG_PAIRS), d_R(pl, SLOT_SG_R), d_trace(pl, SLOT_SG_TRACE), d_end(pl, SLOT_SG_END), d_ops(pl, SLOT_SG_OPS),
            d_cnt(pl, SLOT_SG_CNT), d_res(pl, SLOT_SG_RES), d_off(pl, SLOT_SG_OFF), d_dense(pl, SLOT_SG_DENSE), d_bound(pl, SLOT_SG_BOUND);
        int rc;
        if ((rc = d_pairs.alloc(nb * sizeof(SgPair))) || (rc = d_R.alloc(nb * 4)) || (rc = d_trace.alloc(tbytes)) ||
            (rc = d_end.alloc((nb + 1) * 16)) || (rc = d_ops.alloc(oslots * 4)) || (rc = d_cnt.alloc(nb * 4)) || (rc = d_res.alloc(nb * 24)) ||
            (rc = d_off.alloc(nb * 8)) || (rc = d_bound.alloc(bslots * 8)))
            return rc;
        hc.lap("sg: batch records, scratch");
        ISO_HIP_CHECK(copy_h2d(d_pairs.p, hp.data(), nb * sizeof(SgPair)));
        ISO_HIP_CHECK(copy_h2d(d_R.p, hR.data(), nb * 4));
        tm.start();
        if (n_diag < nb)
            launch_sg_forward_R(general, s->dev, d_pairs.as<SgPair>(), prm, d_trace.as<uint8_t>(), d_bound.as<int2>(),
                                d_end.as<int32_t>(), (unsigned)nb);
        ISO_HIP_CHECK(hipGetLastError());
        // (the kernels of the other classes return at once on a pair that is not theirs; the batch is sorted by cost, so the classes interleave)
        // the narrow tries that do not certify themselves run again inside their wave; counter: the slot behind the last pair's end cell
        uint32_t *d_again = reinterpret_cast<uint32_t *>(d_end.as<int32_t>() + nb * 4);
        if (n_try) ISO_HIP_CHECK(hipMemsetAsync(d_again, 0, 4, 0));
        if (n_diag > n_diag2) launch_sg_band<4>(general, s->dev, d_pairs.as<SgPair>(), prm, d_trace.as<uint8_t>(), d_end.as<int32_t>(), (unsigned)nb, d_again);
        ISO_HIP_CHECK(hipGetLastError());
        if (n_diag2) launch_sg_band<2>(general, s->dev, d_pairs.as<SgPair>(), prm, d_trace.as<uint8_t>(), d_end.as<int32_t>(), (unsigned)nb, d_again);
        ISO_HIP_CHECK(hipGetLastError());
        tm.mark();
        g_sg_stats[4] += (double)n_diag; g_sg_stats[5] += (double)(nb - n_diag); g_sg_stats[7] += (double)tbytes; g_sg_stats[8] += (double)n_diag2;
        if (n_diag < nb)
            hipLaunchKernelGGL(k_sg_walk<0>, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, 0, s->dev, d_pairs.as<SgPair>(), d_R.as<int32_t>(),
                               d_trace.as<uint8_t>(), d_end.as<int32_t>(), d_ops.as<uint32_t>(), d_cnt.as<uint32_t>(), d_res.as<int32_t>(),
                               (uint32_t)nb);
        ISO_HIP_CHECK(hipGetLastError());
        if (n_diag)
            hipLaunchKernelGGL(k_sg_walk_band, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, 0, s->dev, d_pairs.as<SgPair>(), d_trace.as<uint8_t>(),
                               d_end.as<int32_t>(), d_ops.as<uint32_t>(), d_cnt.as<uint32_t>(), d_res.as<int32_t>(), (uint32_t)nb);
        ISO_HIP_CHECK(hipGetLastError());
        tm.stop();
        hc.lap("sg: upload, launches");
        std::vector<uint32_t> cnt(nb);
        ISO_HIP_CHECK(copy_d2h(cnt.data(), d_cnt.p, nb * 4));
        if (n_try) {
            uint32_t again = 0;
            ISO_HIP_CHECK(copy_d2h(&again, d_again, 4));
            g_sg_stats[9] += (double)n_try; g_sg_stats[10] += (double)again;
        }
        hc.lap("sg: kernels (wait for counts)");
        std::vector<int32_t> res(nb * 6);
        ISO_HIP_CHECK(copy_d2h(res.data(), d_res.p, nb * 24));
        const size_t redo_before = redo.size();
        for (size_t i = 0; i < nb; ++i) {
            const uint64_t p = order[pos + i];
            memcpy(out_res + p * 6, res.data() + i * 6, 24);
            if (banded && Xof[p] >= 0) {     // certificate: nothing outside the band can score this much
                const int64_t mn = std::min<int64_t>(lens[a[p]], lens[b[p]]);
                if (!((int64_t)res[i * 6] > (int64_t)match * (mn - Xof[p] - 1))) { redo.push_back(p); g_sg_stats[6] += 1; }
            }
        }
        // The whole call as ONE batch with nothing to redo (the common case: <= 65 536 pairs with good hints): the ops are compacted in PAIR
        // order, straight to their final offsets, and leave the device in one copy into the caller's buffer (no batch buffer, no copy per pair)
        const bool whole_call = round == 0 && pos == 0 && end == order.size() && order.size() == n_pairs && redo.size() == redo_before && redo.empty();
        std::vector<uint64_t> off(nb + 1, 0);
        if (whole_call) {
            out_ops_ptr[0] = 0;
            for (size_t i = 0; i < nb; ++i) out_ops_ptr[order[i] + 1] = cnt[i];
            for (uint64_t p = 0; p < n_pairs; ++p) out_ops_ptr[p + 1] += out_ops_ptr[p];
            ops_direct = out_ops_ptr[n_pairs] <= ops_cap;
        }
        if (ops_direct) {
            for (size_t i = 0; i < nb; ++i) off[i] = out_ops_ptr[order[i]];
            off[nb] = out_ops_ptr[n_pairs];
        } else {
            for (size_t i = 0; i < nb; ++i) off[i + 1] = off[i] + cnt[i];
        }
        if ((rc = d_dense.alloc(off[nb] * 4))) return rc;
        ISO_HIP_CHECK(copy_h2d(d_off.p, off.data(), nb * 8));
        tm_compact.start();
        hipLaunchKernelGGL(k_sg_compact, dim3((unsigned)nb), dim3(256), 0, 0, d_pairs.as<SgPair>(), s->dev, d_ops.as<uint32_t>(),
                           d_cnt.as<uint32_t>(), d_off.as<uint64_t>(), d_dense.as<uint32_t>(), (uint32_t)nb);
        ISO_HIP_CHECK(hipGetLastError());
        tm_compact.stop();
        if (ops_direct) {
            if (off[nb]) ISO_HIP_CHECK(copy_d2h(out_ops, d_dense.p, off[nb] * 4));
        } else {
            batch_ops.emplace_back(off[nb]);
            std::vector<uint32_t> &dense = batch_ops.back();
            if (off[nb]) ISO_HIP_CHECK(copy_d2h(dense.data(), d_dense.p, off[nb] * 4));
            for (size_t i = 0; i < nb; ++i) ops_ref[order[pos + i]] = OpsRef{(uint32_t)(batch_ops.size() - 1), cnt[i], off[i]};
        }
        hc.lap("sg: compact, ops + results down");
        // The whole call as ONE batch with nothing to redo (the common case: <= 65 536 pairs with good hints): the strings are expanded
        // at their final offsets (pair order) and leave the device in one copy straight into the caller's buffers -- no intermediate
        // host copy, no per-pair memcpy (2 x 130 MB at C3).
        if (want_strings && round == 0 && pos == 0 && end == order.size() && order.size() == n_pairs && redo.empty()) {
            std::vector<uint64_t> len_of(n_pairs, 0);
            for (size_t i = 0; i < nb; ++i) len_of[order[i]] = (uint64_t)res[i * 6 + 3] + res[i * 6 + 4] + res[i * 6 + 5];
            out_aln_ptr[0] = 0;
            for (uint64_t p = 0; p < n_pairs; ++p) out_aln_ptr[p + 1] = out_aln_ptr[p] + len_of[p];
            const uint64_t atotal = out_aln_ptr[n_pairs];
            if (atotal <= aln_cap) {
                std::vector<uint64_t> aoff(nb);
                for (size_t i = 0; i < nb; ++i) aoff[i] = out_aln_ptr[order[i]];
                DevBuf d_aoff(pl, SLOT_SG_AOFF), d_alna(pl, SLOT_SG_ALNA), d_alnb(pl, SLOT_SG_ALNB);
                if ((rc = d_aoff.alloc(nb * 8)) || (rc = d_alna.alloc(atotal)) || (rc = d_alnb.alloc(atotal))) return rc;
                ISO_HIP_CHECK(copy_h2d(d_aoff.p, aoff.data(), nb * 8));
                tm_expand.start();
                hipLaunchKernelGGL(k_sg_expand, dim3((unsigned)nb), dim3(256), (1024 + 1) * 3 * 4, 0, s->dev, d_pairs.as<SgPair>(), d_ops.as<uint32_t>(),
                                   d_cnt.as<uint32_t>(), d_aoff.as<uint64_t>(), d_alna.as<uint8_t>(), d_alnb.as<uint8_t>(), (uint32_t)nb);
                ISO_HIP_CHECK(hipGetLastError());
                tm_expand.stop();
                if (atotal) {
                    ISO_HIP_CHECK(copy_d2h(out_aln_a, d_alna.p, atotal));
                    ISO_HIP_CHECK(copy_d2h(out_aln_b, d_alnb.p, atotal));
                }
                strings_direct = true;
                pos = end;
                continue;
            }
        }
        if (want_strings) {
            std::vector<uint64_t> aoff(nb + 1, 0);
            for (size_t i = 0; i < nb; ++i) aoff[i + 1] = aoff[i] + (uint64_t)res[i * 6 + 3] + res[i * 6 + 4] + res[i * 6 + 5];
            DevBuf d_aoff(pl, SLOT_SG_AOFF), d_alna(pl, SLOT_SG_ALNA), d_alnb(pl, SLOT_SG_ALNB);
            if ((rc = d_aoff.alloc(nb * 8)) || (rc = d_alna.alloc(aoff[nb])) || (rc = d_alnb.alloc(aoff[nb]))) return rc;
            ISO_HIP_CHECK(copy_h2d(d_aoff.p, aoff.data(), nb * 8));
            tm_expand.start();
            hipLaunchKernelGGL(k_sg_expand, dim3((unsigned)nb), dim3(256), (1024 + 1) * 3 * 4, 0, s->dev, d_pairs.as<SgPair>(), d_ops.as<uint32_t>(),
                               d_cnt.as<uint32_t>(), d_aoff.as<uint64_t>(), d_alna.as<uint8_t>(), d_alnb.as<uint8_t>(), (uint32_t)nb);
            ISO_HIP_CHECK(hipGetLastError());
            tm_expand.stop();
            batch_a.emplace_back(new uint8_t[aoff[nb] + 1]);
            batch_b.emplace_back(new uint8_t[aoff[nb] + 1]);
            if (aoff[nb]) {
                ISO_HIP_CHECK(copy_d2h(batch_a.back().get(), d_alna.p, aoff[nb]));
                ISO_HIP_CHECK(copy_d2h(batch_b.back().get(), d_alnb.p, aoff[nb]));
            }
            for (size_t i = 0; i < nb; ++i)
                aln_ref[order[pos + i]] = AlnRef{(uint32_t)(batch_a.size() - 1), aoff[i], aoff[i + 1] - aoff[i]};
        }
        pos = end;
    }
  }   // rounds: banded, then the uncertified pairs in full
    hc.lap("sg: certificates, strings");
    uint64_t total = 0;
    if (ops_direct) total = out_ops_ptr[n_pairs];
    else {
        out_ops_ptr[0] = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) { total += ops_ref[p].cnt; out_ops_ptr[p + 1] = total; }
    }
    if (n_ops_needed) *n_ops_needed = total;
    if (kernel_ms) *kernel_ms = tm.total + tm_compact.total + tm_expand.total;
    g_sg_stats[0] = tm.total - tm.marked_total; g_sg_stats[1] = tm.marked_total; g_sg_stats[2] = tm_compact.total; g_sg_stats[3] = tm_expand.total;
    uint64_t atotal = 0;
    if (want_strings && strings_direct) {
        atotal = out_aln_ptr[n_pairs];
        if (n_aln_needed) *n_aln_needed = atotal;
    } else if (want_strings) {
        out_aln_ptr[0] = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) { atotal += aln_ref[p].len; out_aln_ptr[p + 1] = atotal; }
        if (n_aln_needed) *n_aln_needed = atotal;
    }
    if (total > ops_cap || (want_strings && atotal > aln_cap)) return ISOCON_E_CAPACITY;
    if (!ops_direct)
        for (uint64_t p = 0; p < n_pairs; ++p)
            if (ops_ref[p].cnt) memcpy(out_ops + out_ops_ptr[p], batch_ops[ops_ref[p].batch].data() + ops_ref[p].off, (size_t)ops_ref[p].cnt * 4);
    if (want_strings && !strings_direct)
        for (uint64_t p = 0; p < n_pairs; ++p)
            if (aln_ref[p].len) {
                memcpy(out_aln_a + out_aln_ptr[p], batch_a[aln_ref[p].batch].get() + aln_ref[p].off, aln_ref[p].len);
                memcpy(out_aln_b + out_aln_ptr[p], batch_b[aln_ref[p].batch].get() + aln_ref[p].off, aln_ref[p].len);
            }
    hc.lap("sg: ops into the caller's buffer");
    return ISOCON_OK;
}
}  // namespace

extern "C" int isocon_sg_trace_batch(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t match,
                                     const int8_t *mismatch_per_pair, int32_t open, int32_t ext, int32_t tie_policy,
                                     uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *n_ops_needed,
                                     int32_t *out_res, float *kernel_ms, const int32_t *ed_upper)
{
    return sg_batch_impl(s, a, b, n_pairs, match, mismatch_per_pair, open, ext, tie_policy, out_ops, out_ops_ptr, ops_cap,
                         n_ops_needed, out_res, kernel_ms, nullptr, nullptr, nullptr, 0, nullptr, ed_upper);
}

extern "C" int isocon_sg_strings_batch(isocon_store *s, const uint32_t *a, const uint32_t *b, uint64_t n_pairs, int32_t match,
                                       const int8_t *mismatch_per_pair, int32_t open, int32_t ext, int32_t tie_policy,
                                       uint32_t *out_ops, uint64_t *out_ops_ptr, uint64_t ops_cap, uint64_t *n_ops_needed,
                                       int32_t *out_res, uint8_t *out_aln_a, uint8_t *out_aln_b, uint64_t *out_aln_ptr,
                                       uint64_t aln_cap, uint64_t *n_aln_needed, float *kernel_ms, const int32_t *ed_upper)
{
    if (!out_aln_ptr || (aln_cap && (!out_aln_a || !out_aln_b))) return ISOCON_E_ARG;
    return sg_batch_impl(s, a, b, n_pairs, match, mismatch_per_pair, open, ext, tie_policy, out_ops, out_ops_ptr, ops_cap,
                         n_ops_needed, out_res, kernel_ms, out_aln_a, out_aln_b, out_aln_ptr, aln_cap, n_aln_needed, ed_upper);
}

extern "C" int isocon_sg_last_stats(double *out, int32_t cap) { return copy_last_stats(g_sg_stats, 11, out, cap); }

// functions.filter_exon_differences (/root/reference/modules/functions.py:23-50 with get_mask_start_and_end :218-236)
// evaluated on CIGAR ops instead of on the gapped strings: flag[p] = 1 iff one of the two gapped strings has a run of
// >= min_exon_diff '-' inside [start, end), start = min(ignore_ends_len, leading gap run), end = max(len - ignore_ends_len,
// start of the trailing gap run).  'D' ops are the '-' runs of the first (query) string, 'I' ops those of the second.
// Pure host code (no GPU involved).
extern "C" int isocon_exon_filter_from_ops(const uint32_t *ops, const uint64_t *ops_ptr, uint64_t n_pairs, int32_t min_exon_diff,
                                           int32_t ignore_ends_len, uint8_t *out_flag)
{
    if ((n_pairs && (!ops_ptr || !out_flag)) || min_exon_diff < 1 || ignore_ends_len < 0) return ISOCON_E_ARG;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint32_t *o = ops + ops_ptr[p];
        const uint64_t cnt = ops_ptr[p + 1] - ops_ptr[p];
        int64_t A = 0;
        for (uint64_t k = 0; k < cnt; ++k) A += o[k] >> 4;
        int64_t mask_start = 0, mask_end = A;
        if (cnt) {
            if ((o[0] & 15u) >= 2) mask_start = o[0] >> 4;
            if ((o[cnt - 1] & 15u) >= 2) mask_end = A - (int64_t)(o[cnt - 1] >> 4);
        }
        const int64_t start = std::min<int64_t>(ignore_ends_len, mask_start);
        const int64_t end = std::max<int64_t>(A - ignore_ends_len, mask_end);
        uint8_t flag = 0;
        int64_t c = 0;
        for (uint64_t k = 0; k < cnt && !flag; ++k) {
            const int64_t len = o[k] >> 4;
            if ((o[k] & 15u) >= 2) {
                const int64_t lo = std::max(start, c), hi = std::min(end, c + len);
                if (hi - lo >= min_exon_diff) flag = 1;
            }
            c += len;
        }
        out_flag[p] = flag;
    }
    return ISOCON_OK;
}
