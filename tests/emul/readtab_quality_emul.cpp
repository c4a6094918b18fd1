// CPU driver of the base-quality part of isocon_amd/csrc/readtab_core.hpp (tests/test_readtab_quality_core.py): k_rt_read_prefix and
// k_rt_quality (readtab.hpp) with 64 emulated lanes, on tables built by the emulated k_rt_build of readtab_emul.cpp (included: one
// library holds both).
#include "readtab_emul.cpp"

extern "C" {

// k_rt_read_prefix for every row: the gap mask of the read's row and the read bases before each block
void rt_emul_read_prefix(const uint8_t *read, const uint64_t *row_ptr, const uint64_t *blk_ptr, uint32_t n_rows, uint64_t *rgap, uint32_t *rpre)
{
    for (uint32_t r = 0; r < n_rows; ++r) {
        const uint64_t off = row_ptr[r], blk0 = blk_ptr[r];
        const int64_t len = (int64_t)(row_ptr[r + 1] - off), nb = (len + 63) >> 6;
        uint32_t bases = 0;
        for (int64_t b = 0; b < nb; ++b) {
            const int n = len - b * 64 < 64 ? (int)(len - b * 64) : 64;
            const uint64_t gb = ballot([&](int lane) { const int64_t col = b * 64 + lane; return col < len && read[off + col] == '-'; });
            rgap[blk0 + b] = gb;
            rpre[blk0 + b] = bases;
            bases += (uint32_t)popc64(~gb & rt_low_mask(n));
        }
    }
}

// rt_read_bases_upto of one row (rgap / rpre: the row's blocks)
int64_t rt_emul_read_bases_upto(const uint64_t *rgap, const uint32_t *rpre, int64_t pos)
{
    const RtRow R{nullptr, nullptr, nullptr, nullptr, 0, 0, rgap, rpre};
    return rt_read_bases_upto(R, pos);
}

// k_rt_quality for every query (var_pos already wrapped into [0, ref_len)): out_codes[code_ptr[q] + v rows + j]
void rt_emul_quality(const uint64_t *row_ptr, const uint64_t *blk_ptr, const uint64_t *nob, const uint64_t *diff, const uint32_t *pre, const uint8_t *read,
                     const uint32_t *first_row, const uint64_t *rgap, const uint32_t *rpre, const uint8_t *qual, const uint64_t *qual_ptr, const uint32_t *rec_start,
                     uint32_t n_queries, const uint32_t *q_table, const uint8_t *q_kind, const uint64_t *var_ptr, const uint32_t *var_pos, const int32_t *var_u,
                     const uint8_t *var_type, const uint64_t *snip_ptr, const uint8_t *snip_bytes, const uint64_t *code_ptr, uint8_t *out_codes)
{
    for (uint32_t q = 0; q < n_queries; ++q) {
        const uint32_t k = q_table[q], r0 = first_row[k], nr = first_row[k + 1] - r0;
        const uint64_t v0 = var_ptr[q], v1 = var_ptr[q + 1], c0 = code_ptr[q];
        for (int lane = 0; lane < 64; ++lane)
            for (uint32_t j = (uint32_t)lane; j < nr; j += 64) {
                const uint64_t r = (uint64_t)r0 + j, off = row_ptr[r], blk0 = blk_ptr[r], q0 = qual_ptr[r];
                const RtRow R{nob + blk0, diff + blk0, pre + blk0, read + off, (uint32_t)(blk_ptr[r + 1] - blk0), (int64_t)(row_ptr[r + 1] - off), rgap + blk0, rpre + blk0};
                for (uint64_t v = v0; v < v1; ++v)
                    out_codes[c0 + (v - v0) * nr + j] = rt_quality_code(R, var_pos[v], var_u[v], var_type[v], q_kind[q], snip_bytes + snip_ptr[v], snip_ptr[v + 1] - snip_ptr[v],
                                                                        qual + q0, (int64_t)(qual_ptr[r + 1] - q0), rec_start[r]);
            }
    }
}

}  // extern "C"
