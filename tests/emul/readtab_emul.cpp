// CPU driver of isocon_amd/csrc/readtab_core.hpp (tests/test_readtab_core.py): the lane math of the device read tables with 64
// emulated lanes -- a ballot is a loop over the lanes' predicates -- in the shape of k_rt_build / k_rt_support (readtab.hpp).
#include <cstdint>

#include "../../isocon_amd/csrc/readtab_core.hpp"

using namespace isocon;

namespace {

template <class Pred>
uint64_t ballot(Pred p)
{
    uint64_t m = 0;
    for (int lane = 0; lane < 64; ++lane)
        if (p(lane)) m |= 1ull << lane;
    return m;
}

bool symbol_ok(uint8_t ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == '-'; }

}  // namespace

extern "C" {

int rt_emul_select_zero(uint64_t mask, int n) { return rt_select_zero(mask, n); }
uint64_t rt_emul_window(uint64_t w0, uint64_t w1, int sh, int n) { return rt_window(w0, w1, sh, n); }
uint64_t rt_emul_range_mask(int64_t b, int64_t lo, int64_t hi) { return rt_range_mask(b, lo, hi); }
uint32_t rt_emul_find_block(const uint32_t *pre, uint32_t nb, uint32_t i) { return rt_find_block(pre, nb, i); }
int rt_emul_lead_ones(uint64_t m, int n) { return rt_lead_ones(m, n); }
int rt_emul_trail_ones(uint64_t m, int n) { return rt_trail_ones(m, n); }

// k_rt_build for every row: masks and prefix counts per block (blk_ptr: blocks before each row, from the caller), out[4 r ..] =
// insertions, deletions, substitutions, candidate bases.  Returns 1 if a byte outside ACGT- was seen.
int rt_emul_build(const uint8_t *ref, const uint8_t *read, const uint64_t *row_ptr, const uint64_t *blk_ptr, uint32_t n_rows, uint64_t *nob, uint64_t *diff,
                  uint32_t *pre, uint32_t *out)
{
    int bad = 0;
    for (uint32_t r = 0; r < n_rows; ++r) {
        const uint64_t off = row_ptr[r], blk0 = blk_ptr[r];
        const int64_t len = (int64_t)(row_ptr[r + 1] - off), nb = (len + 63) >> 6;
        RtRuns ra = rt_runs_init(), rb = rt_runs_init();
        uint32_t bases = 0;
        auto masks = [&](int64_t b, uint64_t &ga, uint64_t &gb, uint64_t &d) {
            ga = ballot([&](int lane) { const int64_t col = b * 64 + lane; return col < len && ref[off + col] == '-'; });
            gb = ballot([&](int lane) { const int64_t col = b * 64 + lane; return col < len && read[off + col] == '-'; });
            d = ballot([&](int lane) { const int64_t col = b * 64 + lane; return col < len && ref[off + col] != read[off + col]; });
        };
        for (int64_t b = 0; b < nb; ++b) {
            const int n = len - b * 64 < 64 ? (int)(len - b * 64) : 64;
            uint64_t ga, gb, d;
            masks(b, ga, gb, d);
            if (ballot([&](int lane) { const int64_t col = b * 64 + lane; return col < len && !(symbol_ok(ref[off + col]) && symbol_ok(read[off + col])); })) bad = 1;
            nob[blk0 + b] = ga | ~rt_low_mask(n);
            diff[blk0 + b] = d;
            pre[blk0 + b] = bases;
            bases += (uint32_t)popc64(~ga & rt_low_mask(n));
            rt_runs_step(ra, ga, n);
            rt_runs_step(rb, gb, n);
        }
        const int64_t start = ra.lead > rb.lead ? ra.lead : rb.lead;
        const int64_t stop = len - (ra.trail > rb.trail ? ra.trail : rb.trail);
        uint32_t ins = 0, dele = 0, sub = 0;
        for (int64_t b = start >> 6; b < nb && b * 64 < stop; ++b) {
            uint64_t ga, gb, d;
            masks(b, ga, gb, d);
            rt_block_errors(ga, gb, d, b, start, stop, ins, dele, sub);
        }
        out[r * 4] = ins; out[r * 4 + 1] = dele; out[r * 4 + 2] = sub; out[r * 4 + 3] = bases;
    }
    return bad;
}

// k_rt_support for every query (var_pos already wrapped into [0, ref_len))
void rt_emul_support(const uint64_t *row_ptr, const uint64_t *blk_ptr, const uint64_t *nob, const uint64_t *diff, const uint32_t *pre, const uint8_t *read,
                     const uint32_t *first_row, uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr, const uint32_t *var_pos,
                     const int32_t *var_u, const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes, const uint64_t *bits_ptr, uint64_t *out_bits,
                     uint32_t *out_count)
{
    for (uint32_t q = 0; q < n_queries; ++q) {
        const uint32_t k = q_table[q], r0 = first_row[k], nr = first_row[k + 1] - r0;
        const uint64_t v0 = var_ptr[q], v1 = var_ptr[q + 1];
        uint32_t count = 0;
        for (uint32_t step = 0; step * 64 < nr; ++step) {
            const uint64_t word = ballot([&](int lane) {
                const uint32_t j = step * 64 + (uint32_t)lane;
                bool ok = j < nr;
                if (ok && v1 > v0) {
                    const uint64_t r = (uint64_t)r0 + j, off = row_ptr[r], blk0 = blk_ptr[r];
                    const RtRow R{nob + blk0, diff + blk0, pre + blk0, read + off, (uint32_t)(blk_ptr[r + 1] - blk0), (int64_t)(row_ptr[r + 1] - off)};
                    for (uint64_t v = v0; v < v1 && ok; ++v)
                        ok = q_kind[q] ? rt_shows(R, var_pos[v], var_u[v], var_type[v] == 'I', snip_bytes + snip_ptr[v], snip_ptr[v + 1] - snip_ptr[v])
                                       : rt_agrees(R, var_pos[v], var_u[v]);
                }
                return ok;
            });
            out_bits[bits_ptr[q] + step] = word;
            count += (uint32_t)popc64(word);
        }
        out_count[q] = count;
    }
}

}  // extern "C"
