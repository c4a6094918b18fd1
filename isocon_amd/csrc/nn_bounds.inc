// nn_bounds.inc -- NNContext::build_bounds (q-gram profiles, row layouts, tile table, k_qgram_mm) and NNContext::run_bound_seeds (the smallest-bound pairs proposed and aligned first) (included by isocon_hip.hip behind nn_context.inc).

namespace {

int NNContext::build_bounds(const QMap &Q, int32_t kcap, NNParams &P, bool want_seeds)
{
    const uint32_t q_begin = Q.begin, q_end = Q.end;
    P.lb = nullptr;
    P.lb_row = nullptr;
    P.slot_order = nullptr;
    if (variant("nn_no_qgram") || n < 2 || n >= (1u << 30) || q_begin >= q_end) return ISOCON_OK;          // (k_qgram_mm keeps offsets inside a tile in 32 bits)
    if (!want_seeds && st->pool.bound_tag.valid && st->pool.bound_tag.serial == st->serial && st->pool.bound_tag.map.same(Q) &&
        st->pool.bound_tag.depth == depth && st->pool.bound_tag.kcap == kcap) {
        // the seed phase of this very store and shard left the matrix in the pool (isocon_nn_partial phase 0 -> phase 1)
        P.lb = static_cast<const uint8_t *>(st->pool.slots[SLOT_NN_LB].p);
        P.lb_row = lb_row_dev = st->pool.bound_tag.lb_row;
        lb_len_dev = st->pool.bound_tag.lb_len;
        if (st->pool.bound_tag.has_order && use_slot_order(Q.count())) P.slot_order = static_cast<const uint32_t *>(st->pool.slots[SLOT_NN_SLOTORDER].p);
        lb_total = st->pool.bound_tag.lb_total;
        return ISOCON_OK;
    }
    st->pool.bound_tag.valid = false;
    const uint32_t nq = Q.count();
    const std::vector<int32_t> &lens = st->lens;
    // the profiles do not depend on the row layout: their kernel runs while the host lays out rows, transposed rows and tiles
    const uint32_t n_pad = std::max<uint32_t>(QM_TILE, ((n + QM_TILE - 1) / QM_TILE) * QM_TILE);
    const size_t prof_bytes = (size_t)n_pad * (QM_K / 2);
    d_qprof.pool = d_qsum.pool = &st->pool;
    d_qprof.slot = SLOT_NN_QPROF; d_qsum.slot = SLOT_NN_QSUM;
    HostClock bclk;
    {
        size_t free_b = 0;
        if (!free_mem(free_b) || prof_bytes > free_b / 2 + st->pool.slots[SLOT_NN_QPROF].cap) return ISOCON_OK;
        if (d_qprof.alloc(prof_bytes) || d_qsum.alloc((size_t)n * 4)) return ISOCON_OK;
    }
    // the step is going to run the block filter: the profile kernel writes its 2-bit texts on the way (no room for them: plan_lists finds
    // none either and runs without the filter)
    uint32_t *text2 = !text2_ready && filter_wanted() && text2_room() ? d_text2.as<uint32_t>() : nullptr;
    bclk.lap("bounds: memory check + profile buffers");
    // What an earlier call left on the side stream is through before anything below is enqueued.  The side stream's work below starts
    // behind everything the null stream holds at this point, not behind the profile kernel.
    g_side.settle();
    const bool side = !variant("nn_sync_uploads") && g_side.ready() && hipEventRecord(g_side.before, 0) == hipSuccess;
    tm.start();
    hipLaunchKernelGGL(k_qgram_profile4, dim3((n + QP_SEQS - 1) / QP_SEQS), dim3(256), 0, 0, st->dev, d_qprof.as<uint8_t>(), d_qsum.as<uint32_t>(), n_pad,
                       text2, text2_stride);
    ISO_HIP_CHECK(hipGetLastError());
    if (text2) text2_ready = true;
    struct StopTimer { NNContext &c; bool armed = true; ~StopTimer() { if (armed) c.tm.stop_later(&c.stats.bound_kernel_ms); } } stop_timer{*this};
    // Everything between the profile kernel and k_qgram_mm that neither of them writes or reads goes on the side stream while the
    // profile kernel runs.  At once, while the host lays out the rows: the fills that are sized from n alone -- the hub scores, the
    // row / column minima, the seed arrays of run_bound_seeds, their counter and the table of the seed pairs.  Behind the host's loops: row lengths, tile table and
    // row offsets (staged in pinned memory) and the transposed matrix' row layout (k_lbt_rows, its scan, k_lbt_offsets).  The null
    // stream waits for all of it once, in front of k_qgram_mm; the host does not wait at all.  Without a side stream the same
    // operations go on the null stream, the uploads as three blocking copies.
    hipStream_t ls = 0;          // the stream of the fills and the row layout
    // an early return between the first side-stream operation and the null stream's wait leaves nothing in flight behind it
    struct SideGuard { bool armed = false; ~SideGuard() { if (armed) g_side.settle(); } } side_guard;
    if (side) {
        g_side.in_flight = side_guard.armed = true;          // (from the first operation on: an error below must not let the next call write the pinned block, or a buffer of the pool, unsettled)
        ISO_HIP_CHECK(hipStreamWaitEvent(g_side.stream, g_side.before, 0));
        ls = g_side.stream;
    }
    d_score.pool = &st->pool;
    d_score.slot = SLOT_NN_SCORE;
    if (d_score.alloc((size_t)n * 4)) return ISOCON_OK;
    QMFills fills = {};
    fills.r[0] = {d_score.as<uint32_t>(), n, 0u};
    unsigned long long *rowmin = nullptr, *colmin = nullptr;
    if (want_seeds) {
        const uint64_t n_seed_words = (uint64_t)2 * QM_SEEDS * n;          // dwords of each of the two seed arrays (run_bound_seeds: np)
        d_rowmin.pool = d_colmin.pool = d_seed_a.pool = d_seed_b.pool = d_seed_n.pool = &st->pool;
        d_rowmin.slot = SLOT_NN_ROWMIN; d_colmin.slot = SLOT_NN_COLMIN; d_seed_a.slot = SLOT_NN_SEED_A; d_seed_b.slot = SLOT_NN_SEED_B; d_seed_n.slot = SLOT_NN_SEED_N;
        if (!(d_rowmin.alloc((size_t)nq * 8 * QM_SEEDS) || d_colmin.alloc((size_t)n_pad * 8 * QM_SEEDS) || d_seed_a.alloc((size_t)n_seed_words * 4) || d_seed_b.alloc((size_t)n_seed_words * 4) ||
              d_seed_n.alloc(8))) {
            fills.r[1] = {d_rowmin.as<uint32_t>(), (unsigned long long)nq * 2 * QM_SEEDS, 0xffffffffu};
            fills.r[2] = {d_colmin.as<uint32_t>(), (unsigned long long)n_pad * 2 * QM_SEEDS, 0xffffffffu};
            fills.r[3] = {d_seed_a.as<uint32_t>(), n_seed_words, 0xffffffffu};
            fills.r[4] = {d_seed_b.as<uint32_t>(), n_seed_words, 0xffffffffu};
            fills.r[5] = {d_seed_n.as<uint32_t>(), 2, 0u};
            // the table of the seed pairs (NNSeedKnown): "none" everywhere; no room for it: the seeds run without, the main pass aligns every pair
            static_assert(NN_KNOWN_SLOTS == 2 * QM_SEEDS, "a table row holds every pair a thread of k_qgram_seed_pairs can propose");
            d_known.pool = &st->pool;
            d_known.slot = SLOT_NN_SEED_KNOWN;
            if (d_known.alloc((size_t)n * NN_KNOWN_SLOTS * 4) == ISOCON_OK) fills.r[6] = {d_known.as<uint32_t>(), (unsigned long long)n * NN_KNOWN_SLOTS, 0xffffffffu};
            else d_known.p = nullptr;
            rowmin = d_rowmin.as<unsigned long long>();
            colmin = d_colmin.as<unsigned long long>();
        }
    }
    hipLaunchKernelGGL(k_qm_fills, dim3(1024), dim3(256), 0, ls, fills);
    ISO_HIP_CHECK(hipGetLastError());
    // Row s of the matrix = launch slot s of the main pass = entry q = Q.entry(s), its columns the neighbours
    // p = q + 1 .. q + rlen[s]; the kernels address column p as lb[off[s] + (p - q - 1)].  A row's storage starts at a 16-byte
    // boundary with column (q + 1) & ~15 and ends with column ((q + rlen) | 15), so the address of column p is congruent to
    // p mod 16 and k_qgram_mm writes whole aligned 16-byte pieces (the pad bytes of a row are its own).
    std::vector<unsigned long long> &off = lb_off_host;
    std::vector<uint32_t> &rlen = lb_len_host;
    off.assign(nq, 0);
    rlen.assign(nq, 0);
    unsigned long long total = 0, sum_rlen = 0;
    uint64_t hi = 0;
    const uint32_t nrb = (nq + QM_TILE - 1) / QM_TILE;             // row blocks of 256 slots
    std::vector<uint64_t> rb_lo(nrb, ~(uint64_t)0), rb_hi(nrb, 0);        // first / last column of a row block
    for (uint32_t s = 0; s < nq; ++s) {
        const uint64_t q = Q.entry(s);
        if (hi < q + 1) hi = q + 1;
        while (hi < n && lens[hi] - lens[q] <= kcap) ++hi;          // lens ascend: hi only moves forward
        uint64_t len = hi - q - 1;
        if (len > depth) len = depth;
        const uint64_t pal = (q + 1) & ~(uint64_t)15;
        off[s] = total + (q + 1 - pal);
        rlen[s] = (uint32_t)len;
        sum_rlen += len;
        if (len) {
            total += ((q + 1 + len + 15) & ~(uint64_t)15) - pal;
            rb_lo[s / QM_TILE] = std::min<uint64_t>(rb_lo[s / QM_TILE], q + 1);
            rb_hi[s / QM_TILE] = std::max<uint64_t>(rb_hi[s / QM_TILE], q + len);
        }
    }
    if (total == 0) return ISOCON_OK;
    bclk.lap("bounds: profile launch + rows (host)");
    // The transposed matrix: row p holds the slots whose window contains p (s with q(s) < p <= q(s) + rlen[s]: a contiguous range,
    // both ends ascend with p), lbT[offT[p] + (s - sloT[p])], storage from slot sloT & ~15 so that the address is congruent to s mod 16.
    // Its row layout (sloT, lenT, offT) is computed on the device (k_lbt_rows + a scan, below: 1.2 ms of host loop at 50 000
    // entries otherwise, which a rank of a sharded search cannot hide behind its short bound kernel); the host only needs an upper
    // bound of its size: the cells are those of the matrix, a row pads at most 30 bytes.
    const unsigned long long totalT = sum_rlen + 30ull * n;
    bclk.lap("bounds: transposed rows (host)");
    size_t free_b = 0;
    const size_t need = (size_t)total + (size_t)totalT + prof_bytes + (size_t)n * 24 + (size_t)nq * 12;
    if (!free_mem(free_b) || need > free_b / 2 + st->pool.slots[SLOT_NN_LB].cap + st->pool.slots[SLOT_NN_QPROF].cap) return ISOCON_OK;
    // Tile table of k_qgram_mm: 256 x 256 tiles in super-tiles of 4 row blocks x 8 column blocks = 32 entries (0xffffffff = no
    // tile); the kernel hands the 32 entries of a super-tile to workgroups that share an XCD, so a super-tile loads 12 operand
    // panels from beyond L2 instead of 64.
    bclk.lap("bounds: memory check 2");
    std::vector<uint2> tiles;
    for (uint32_t g = 0; g * 4 < nrb; ++g) {
        uint64_t jmin = ~(uint64_t)0, jmax = 0;
        bool any = false;
        for (uint32_t I = g * 4; I < std::min(nrb, g * 4 + 4); ++I)
            if (rb_lo[I] != ~(uint64_t)0) { any = true; jmin = std::min(jmin, rb_lo[I] / QM_TILE); jmax = std::max(jmax, rb_hi[I] / QM_TILE); }
        if (!any) continue;
        for (uint64_t j0 = jmin; j0 <= jmax; j0 += 8)
            for (uint32_t ri = 0; ri < 4; ++ri)
                for (uint32_t cj = 0; cj < 8; ++cj) {
                    const uint32_t I = g * 4 + ri;
                    const uint64_t J = j0 + cj;
                    const bool have = I < nrb && rb_lo[I] != ~(uint64_t)0 && J >= rb_lo[I] / QM_TILE && J <= rb_hi[I] / QM_TILE;
                    tiles.push_back(have ? make_uint2(I, (uint32_t)J) : make_uint2(0xffffffffu, 0xffffffffu));
                }
    }
    while (tiles.size() % 256) tiles.push_back(make_uint2(0xffffffffu, 0xffffffffu));
    if (tiles.size() > 0x7fffffffull) return ISOCON_OK;
    bclk.lap("bounds: tile table (host)");
    d_lb.pool = &st->pool;
    d_lb.slot = SLOT_NN_LB;
    int rc;
    if ((rc = d_lb.alloc((size_t)total + 16))) return ISOCON_OK;          // no room: the pass runs without bounds (16 spare bytes, as behind the transposed matrix: the list builder reads whole dwords at a row's end)
    d_lbt.pool = d_offT.pool = d_sloT.pool = d_lenT.pool = &st->pool;
    d_lbt.slot = SLOT_NN_LBT; d_offT.slot = SLOT_NN_LBT_OFF; d_sloT.slot = SLOT_NN_LBT_SLO; d_lenT.slot = SLOT_NN_LBT_LEN;
    DevBuf d_padT(&st->pool, SLOT_NN_LBT_PAD);
    if (d_lbt.alloc((size_t)totalT + 16) || d_offT.alloc(((size_t)n + 1) * 8) || d_sloT.alloc((size_t)n * 4) || d_lenT.alloc((size_t)n * 4) ||
        d_padT.alloc((size_t)n * 4))
        return ISOCON_OK;
    d_chunks.pool = &st->pool;
    d_chunks.slot = SLOT_NN_LBCHUNKS;
    // tile table, row offsets and row lengths: one buffer on the device, laid out like the pinned block, so that they go up in ONE copy
    // (three copies on the side stream took 70 us from the first start to the last end, 28 us of them copying)
    const size_t b_tiles = (tiles.size() * sizeof(uint2) + 15) & ~(size_t)15, b_off = ((size_t)nq * 8 + 15) & ~(size_t)15, b_len = (size_t)nq * 4;
    if (d_chunks.alloc(b_tiles + b_off + b_len)) return ISOCON_OK;
    unsigned long long *const d_lbrow = reinterpret_cast<unsigned long long *>(d_chunks.as<char>() + b_tiles);
    uint32_t *const d_lblen = reinterpret_cast<uint32_t *>(d_chunks.as<char>() + b_tiles + b_off);
    char *pin = nullptr;
    if (side) pin = static_cast<char *>(g_side.pinned.get(b_tiles + b_off + b_len));
    if (pin) {
        memcpy(pin, tiles.data(), tiles.size() * sizeof(uint2));
        memcpy(pin + b_tiles, off.data(), (size_t)nq * 8);
        memcpy(pin + b_tiles + b_off, rlen.data(), (size_t)nq * 4);
        ISO_HIP_CHECK(hipMemcpyAsync(d_chunks.p, pin, b_tiles + b_off + b_len, hipMemcpyHostToDevice, ls));
    } else {
        ISO_HIP_CHECK(copy_h2d(d_chunks.p, tiles.data(), tiles.size() * sizeof(uint2)));
        ISO_HIP_CHECK(copy_h2d(d_lbrow, off.data(), (size_t)nq * 8));
        ISO_HIP_CHECK(copy_h2d(d_lblen, rlen.data(), (size_t)nq * 4));
    }
    hipLaunchKernelGGL(k_lbt_rows, dim3((n + 255) / 256), dim3(256), 0, ls, Q, nq, d_lblen, n, d_sloT.as<uint32_t>(), d_lenT.as<uint32_t>(), d_padT.as<uint32_t>());
    if ((rc = device_exscan<0, unsigned long long>(&st->pool, d_padT.as<uint32_t>(), n, d_offT.as<unsigned long long>(), ls))) return ISOCON_OK;
    hipLaunchKernelGGL(k_lbt_offsets, dim3((n + 255) / 256), dim3(256), 0, ls, n, d_sloT.as<uint32_t>(), d_offT.as<unsigned long long>());
    ISO_HIP_CHECK(hipGetLastError());
    if (ls) ISO_HIP_CHECK(hipEventRecord(g_side.done, ls));
    bclk.lap("bounds: alloc + uploads + row layout (enqueued)");
    if (use_slot_order(nq)) {
        // workgroup order of the main pass: widest windows first (stable sort by row length), so that the launch does
        // not end with a few long-running entries -- matters when a rank's share is only a few rounds of workgroups
        std::vector<uint32_t> order(nq);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rlen[x] > rlen[y]; });
        d_order.pool = &st->pool;
        d_order.slot = SLOT_NN_SLOTORDER;
        if (d_order.alloc((size_t)nq * 4)) return ISOCON_OK;
        ISO_HIP_CHECK(copy_h2d(d_order.p, order.data(), (size_t)nq * 4));
    }
    bclk.lap("bounds: slot order");
    static bool lds_attr_set = false;
    if (!lds_attr_set) {
        ISO_HIP_CHECK(hipFuncSetAttribute((const void *)k_qgram_mm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QM_LDS_BYTES));
        lds_attr_set = true;
    }
    if (ls) {
        ISO_HIP_CHECK(hipStreamWaitEvent(0, g_side.done, 0));
        side_guard.armed = false;
    }
    tm.mark();          // (the contraction by itself: mm_kernel_ms)
    hipLaunchKernelGGL(k_qgram_mm, dim3((unsigned)tiles.size()), dim3(512), QM_LDS_BYTES, 0, d_qprof.as<uint8_t>(), d_qsum.as<uint32_t>(), n, n_pad,
                       d_chunks.as<uint2>(), d_lbrow, d_lblen, d_lb.as<uint8_t>(), Q, nq,
                       d_qf.as<uint8_t>(), d_tf.as<uint8_t>(), rowmin, colmin, d_offT.as<unsigned long long>(), d_sloT.as<uint32_t>(), d_lenT.as<uint32_t>(),
                       d_lbt.as<uint8_t>(), d_score.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    stop_timer.armed = false;
    tm.stop_later(&stats.bound_kernel_ms, &stats.mm_kernel_ms);          // (the context's own marked time is the narrow table launch's: narrow_kernel_ms)
    bclk.lap("bounds: k_qgram_mm (enqueued)");
#ifdef ISOCON_QM_TIMELINE
    {
        const size_t nt = std::min<size_t>(tiles.size(), 16384);
        std::vector<unsigned long long> tl(nt * 8);
        ISO_HIP_CHECK(hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(g_qm_timeline), nt * 64));
        double sum[5] = {0, 0, 0, 0, 0};
        unsigned long long t_min = ~0ull, t_max = 0;
        size_t cnt = 0;
        for (size_t b = 0; b < nt; ++b) {
            if (tiles[b].x == 0xffffffffu) continue;
            const unsigned long long *t = tl.data() + b * 8;
            for (int k = 0; k < 5; ++k) sum[k] += (double)(t[k + 1] - t[k]);
            t_min = std::min(t_min, t[0]); t_max = std::max(t_max, t[5]);
            ++cnt;
        }
        // s_memtime ticks at 100 MHz on this part
        fprintf(stderr, "[qm timeline] %zu tiles: prologue %.2f us, K loop %.2f us, E1 %.2f us, E2 %.2f us, E3 %.2f us per tile; first start to last end %.3f ms\n", cnt,
                sum[0] / cnt / 100.0, sum[1] / cnt / 100.0, sum[2] / cnt / 100.0, sum[3] / cnt / 100.0, sum[4] / cnt / 100.0, (double)(t_max - t_min) / 1e5);
    }
#endif
    for (const uint2 &t : tiles) stats.bound_tiles += t.x != 0xffffffffu;
    P.lb = d_lb.as<uint8_t>();
    P.lb_row = lb_row_dev = d_lbrow;
    lb_len_dev = d_lblen;
    if (use_slot_order(nq)) P.slot_order = d_order.as<uint32_t>();
    seeds_ready = rowmin != nullptr;
    seed_nq = nq;
    lb_total = total;
    st->pool.bound_tag.valid = true;
    st->pool.bound_tag.lb_total = total;
    st->pool.bound_tag.lb_row = d_lbrow;
    st->pool.bound_tag.lb_len = d_lblen;
    st->pool.bound_tag.has_order = use_slot_order(nq);
    st->pool.bound_tag.serial = st->serial;
    st->pool.bound_tag.map = Q; st->pool.bound_tag.depth = depth; st->pool.bound_tag.kcap = kcap;
    return ISOCON_OK;
}

// The seed pairs of the shard from the row / column minima build_bounds left (k_qgram_seed_pairs): appended to d_seed_a / d_seed_b, counted in
// d_seed_n, each entry's pairs in its row of the known table.  classes_used: the col_classes of the launch.
int NNContext::propose_bound_seeds(const QMap &Q, uint32_t *classes_used)
{
    // a shard that owns 1 / N of the rows merges its column candidates into QM_SEEDS / N classes (k_qgram_seed_pairs)
    const uint32_t ranks = std::max<uint32_t>(1u, Q.stride >> Q.block_log2);
    uint32_t col_classes = QM_SEEDS;
    while (col_classes > 1 && col_classes * ranks > (uint32_t)QM_SEEDS) col_classes >>= 1;
    if (const char *e = variant_value("nn_seed_classes")) { const int v = atoi(e); if (v == 1 || v == 2 || v == QM_SEEDS) col_classes = (uint32_t)v; }      // A/B runs
    // (build_bounds filled the seed arrays and zeroed their counter on its way: seeds_ready says so)
    hipLaunchKernelGGL(k_qgram_seed_pairs, dim3((n + 255) / 256), dim3(256), 0, 0, d_rowmin.as<unsigned long long>(), d_colmin.as<unsigned long long>(),
                       n, Q, seed_nq, col_classes, d_seed_a.as<uint32_t>(), d_seed_b.as<uint32_t>(), d_seed_n.as<unsigned long long>(), d_known.as<uint32_t>());
    ISO_HIP_CHECK(hipGetLastError());
    if (classes_used) *classes_used = col_classes;
    return ISOCON_OK;
}

// Exact distances of the proposed pairs (one pair per lane, ed_lanes.hpp) through the update rule of the search: best[] starts the main
// pass close to its final values.
int NNContext::align_bound_seeds()
{
    const uint64_t np = (uint64_t)2 * QM_SEEDS * n;
    hipLaunchKernelGGL(k_ed_lanes<true>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, 0, st->dev, params(63), d_seed_a.as<uint32_t>(), d_seed_b.as<uint32_t>(),
                       (const int32_t *)nullptr, np, (int32_t *)nullptr);
    ISO_HIP_CHECK(hipGetLastError());
    return ISOCON_OK;
}

// Every entry's smallest-bound pairs aligned first: the proposal, then the alignment.
int NNContext::run_bound_seeds(const QMap &Q)
{
    if (!seeds_ready) return ISOCON_OK;
    tm.start();
    int rc;
    if ((rc = propose_bound_seeds(Q)) || (rc = align_bound_seeds())) return rc;
    tm.stop_later(&stats.seed_kernel_ms);
    known_ready = d_known.p != nullptr;          // (every pair in the table is in the launch above)
    return ISOCON_OK;
}

}  // namespace
