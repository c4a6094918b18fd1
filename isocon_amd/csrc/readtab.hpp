// readtab.hpp -- kernels of the device read tables of the statistical test (isocon_readtab_*: readtab_host.inc; lane math in
// readtab_core.hpp).  Reference call sites: modules/functions.py:149-201 (get_support), :204-216 (get_read_errors), :495-522
// (read_errors_from_alignment), modules/hypothesis_test_module.py:92-171.
//
//   k_rt_build    one wavefront per row, 64 columns per step: the gap masks of both rows and the mask of differing columns are wave
//                 ballots, the count of candidate bases before a block is a running popcount, the end gap runs come from
//                 leading / trailing-zero counts of the gap masks.  A second walk over the row counts the errors between the end runs.
//   k_rt_support  one wavefront per query (one side of one edge), the rows of its table on the lanes in steps of 64; the variant list
//                 is wave-uniform.  A lane finds the block of the variant's candidate base in its row's prefix counts, the column by a
//                 select inside the block's word, and compares its window (reads of c: no differing column; reads of t: the snippet).
//   k_rt_read_prefix  (table sets with base qualities) one wavefront per row, 64 columns per step: the gap mask of the read's row is a
//                 ballot, the count of read bases before a block a running popcount.
//   k_rt_quality  one wavefront per query as in k_rt_support; per variant every lane writes one byte, rt_quality_code of its row: the
//                 quality at the variant's place in the read's record or the reason there is none.  The 64 bytes of a wavefront
//                 and variant are one contiguous run.
//   k_rt_probability  the same walk, but the code bytes stay in the lane: every row keeps (alive, p) in registers over the variant loop
//                 and multiplies its error probability up as the host's _ccs_probabilities_from_codes does, bit for bit
//                 (rt_probability_step); one double per row at the end.  What the host would raise becomes the query's status word: the
//                 minimum of (variant << 2 | rank) over the lanes' rows, by six xor-shuffles after the row loop.
// No LDS, no scratch; lane 0 writes a wavefront's words.
#pragma once
#include "common.hpp"
#include "readtab_core.hpp"

namespace isocon {

struct RtTables {
    const uint64_t *row_ptr;          // n_rows + 1: columns before row r
    const uint64_t *blk_ptr;          // n_rows + 1: 64-column blocks before row r
    const uint64_t *nob, *diff;       // per block (readtab_core.hpp)
    const uint32_t *pre;              // per block
    const uint8_t *read;              // the bytes of the reads' rows
    const uint32_t *first_row;        // n_tables + 1
};

struct RtQueries {
    const uint32_t *q_table;
    const uint8_t *q_kind;
    const uint64_t *var_ptr;
    const uint32_t *var_pos;          // already wrapped into [0, ref_len)
    const int32_t *var_u;
    const uint8_t *var_type;
    const uint64_t *snip_ptr;
    const uint8_t *snip_bytes;
    const uint64_t *out_ptr;          // k_rt_support: first word of the query's bit set, k_rt_quality: first byte of its codes
    uint32_t n;
};

struct RtQualities {                  // what isocon_readtab_set_qualities adds to a table set
    const uint64_t *rgap;             // per block (readtab_core.hpp)
    const uint32_t *rpre;             // per block
    const uint8_t *qual;              // the records' qualities
    const uint64_t *qual_ptr;         // n_rows + 1: qualities before row r's record
    const uint32_t *rec_start;        // n_rows: where the read starts in its record
};

ISO_HD bool rt_symbol_ok(uint8_t ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == '-'; }

// out[4 r ..] = insertions, deletions, substitutions, candidate bases of row r; *bad != 0: some row holds a byte outside ACGT-
__global__ __launch_bounds__(256) void k_rt_build(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ read, const uint64_t *__restrict__ row_ptr,
                                                   const uint64_t *__restrict__ blk_ptr, uint32_t n_rows, uint64_t *__restrict__ nob, uint64_t *__restrict__ diff,
                                                   uint32_t *__restrict__ pre, uint32_t *__restrict__ out, uint32_t *__restrict__ bad)
{
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t off = row_ptr[r], blk0 = blk_ptr[r];
    const int64_t len = (int64_t)(row_ptr[r + 1] - off);
    const int64_t nb = (len + 63) >> 6;
    RtRuns ra = rt_runs_init(), rb = rt_runs_init();
    uint32_t bases = 0;
    bool any_bad = false;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t col = b * 64 + lane;
        const bool in = col < len;
        const uint8_t a = in ? ref[off + col] : (uint8_t)'-', x = in ? read[off + col] : (uint8_t)'-';
        const int n = len - b * 64 < 64 ? (int)(len - b * 64) : 64;
        const uint64_t ga = __ballot(in && a == '-'), gb = __ballot(in && x == '-'), d = __ballot(in && a != x);
        any_bad |= __ballot(in && !(rt_symbol_ok(a) && rt_symbol_ok(x))) != 0;
        if (lane == 0) {
            nob[blk0 + b] = ga | ~rt_low_mask(n);
            diff[blk0 + b] = d;
            pre[blk0 + b] = bases;
        }
        bases += (uint32_t)popc64(~ga & rt_low_mask(n));
        rt_runs_step(ra, ga, n);
        rt_runs_step(rb, gb, n);
    }
    const int64_t start = ra.lead > rb.lead ? ra.lead : rb.lead;
    const int64_t stop = len - (ra.trail > rb.trail ? ra.trail : rb.trail);
    uint32_t ins = 0, dele = 0, sub = 0;
    for (int64_t b = start >> 6; b < nb && b * 64 < stop; ++b) {
        const int64_t col = b * 64 + lane;
        const bool in = col < len;
        const uint8_t a = in ? ref[off + col] : (uint8_t)'-', x = in ? read[off + col] : (uint8_t)'-';
        const uint64_t ga = __ballot(in && a == '-'), gb = __ballot(in && x == '-'), d = __ballot(in && a != x);
        rt_block_errors(ga, gb, d, b, start, stop, ins, dele, sub);
    }
    if (lane == 0) {
        out[r * 4] = ins;
        out[r * 4 + 1] = dele;
        out[r * 4 + 2] = sub;
        out[r * 4 + 3] = bases;
        if (any_bad) *bad = 1u;
    }
}

__global__ __launch_bounds__(256) void k_rt_support(RtTables T, RtQueries Q, uint64_t *__restrict__ out_bits, uint32_t *__restrict__ out_count)
{
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = Q.q_table[q];
    const uint32_t r0 = T.first_row[k], nr = T.first_row[k + 1] - r0;
    const uint64_t v0 = Q.var_ptr[q], v1 = Q.var_ptr[q + 1], w0 = Q.out_ptr[q];
    const bool snippets = Q.q_kind[q] != 0;
    uint32_t count = 0;
    for (uint32_t step = 0; step * 64 < nr; ++step) {
        const uint32_t j = step * 64 + lane;
        bool ok = j < nr;
        if (ok && v1 > v0) {
            const uint64_t r = (uint64_t)r0 + j;
            const uint64_t off = T.row_ptr[r], blk0 = T.blk_ptr[r];
            const RtRow R{T.nob + blk0, T.diff + blk0, T.pre + blk0, T.read + off, (uint32_t)(T.blk_ptr[r + 1] - blk0), (int64_t)(T.row_ptr[r + 1] - off)};
            for (uint64_t v = v0; v < v1 && ok; ++v) {
                if (snippets) ok = rt_shows(R, Q.var_pos[v], Q.var_u[v], Q.var_type[v] == 'I', Q.snip_bytes + Q.snip_ptr[v], Q.snip_ptr[v + 1] - Q.snip_ptr[v]);
                else ok = rt_agrees(R, Q.var_pos[v], Q.var_u[v]);
            }
        }
        const uint64_t word = __ballot(ok);
        if (lane == 0) out_bits[w0 + step] = word;
        count += (uint32_t)popc64(word);
    }
    if (lane == 0) out_count[q] = count;
}

__global__ __launch_bounds__(256) void k_rt_read_prefix(const uint8_t *__restrict__ read, const uint64_t *__restrict__ row_ptr, const uint64_t *__restrict__ blk_ptr,
                                                         uint32_t n_rows, uint64_t *__restrict__ rgap, uint32_t *__restrict__ rpre)
{
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t off = row_ptr[r], blk0 = blk_ptr[r];
    const int64_t len = (int64_t)(row_ptr[r + 1] - off);
    const int64_t nb = (len + 63) >> 6;
    uint32_t bases = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t col = b * 64 + lane;
        const int n = len - b * 64 < 64 ? (int)(len - b * 64) : 64;
        const uint64_t gb = __ballot(col < len && read[off + col] == '-');
        if (lane == 0) {
            rgap[blk0 + b] = gb;
            rpre[blk0 + b] = bases;
        }
        bases += (uint32_t)popc64(~gb & rt_low_mask(n));
    }
}

// out_codes[out_ptr[q] + v nr + j]: variant v (0-based in the query) and row j of the query's table of nr rows
__global__ __launch_bounds__(256) void k_rt_quality(RtTables T, RtQualities U, RtQueries Q, uint8_t *__restrict__ out_codes)
{
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = Q.q_table[q];
    const uint32_t r0 = T.first_row[k], nr = T.first_row[k + 1] - r0;
    const uint64_t v0 = Q.var_ptr[q], v1 = Q.var_ptr[q + 1], c0 = Q.out_ptr[q];
    const int kind = Q.q_kind[q];
    for (uint32_t j = lane; j < nr; j += 64) {
        const uint64_t r = (uint64_t)r0 + j;
        const uint64_t off = T.row_ptr[r], blk0 = T.blk_ptr[r], q0 = U.qual_ptr[r];
        const RtRow R{T.nob + blk0, T.diff + blk0, T.pre + blk0, T.read + off, (uint32_t)(T.blk_ptr[r + 1] - blk0), (int64_t)(T.row_ptr[r + 1] - off), U.rgap + blk0,
                      U.rpre + blk0};
        const int64_t rec_len = (int64_t)(U.qual_ptr[r + 1] - q0), rec_start = U.rec_start[r];
        for (uint64_t v = v0; v < v1; ++v)
            out_codes[c0 + (v - v0) * nr + j] = rt_quality_code(R, Q.var_pos[v], Q.var_u[v], Q.var_type[v], kind, Q.snip_bytes + Q.snip_ptr[v],
                                                                Q.snip_ptr[v + 1] - Q.snip_ptr[v], U.qual + q0, rec_len, rec_start);
    }
}

// out_prob[out_ptr[q] + j]: row j of the query's table -- its probability, -1.0 (not informative) or -2.0 (it raised); out_status[q]:
// rt_prob_status of the smallest event key of the query's rows.  q_ratios: 3 doubles per query, p_of_quality: 94 doubles.
__global__ __launch_bounds__(256) void k_rt_probability(RtTables T, RtQualities U, RtQueries Q, const double *__restrict__ q_ratios,
                                                         const double *__restrict__ p_of_quality, double *__restrict__ out_prob, uint32_t *__restrict__ out_status)
{
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t k = Q.q_table[q];
    const uint32_t r0 = T.first_row[k], nr = T.first_row[k + 1] - r0;
    const uint64_t v0 = Q.var_ptr[q], v1 = Q.var_ptr[q + 1], c0 = Q.out_ptr[q];
    const int kind = Q.q_kind[q];
    const double *ratios = q_ratios + (size_t)q * 3;
    uint32_t first = RT_P_NO_EVENT;          // over this lane's rows of all 64-row passes
    for (uint32_t j = lane; j < nr; j += 64) {
        const uint64_t r = (uint64_t)r0 + j;
        const uint64_t off = T.row_ptr[r], blk0 = T.blk_ptr[r], q0 = U.qual_ptr[r];
        const RtRow R{T.nob + blk0, T.diff + blk0, T.pre + blk0, T.read + off, (uint32_t)(T.blk_ptr[r + 1] - blk0), (int64_t)(T.row_ptr[r + 1] - off), U.rgap + blk0,
                      U.rpre + blk0};
        const int64_t rec_len = (int64_t)(U.qual_ptr[r + 1] - q0), rec_start = U.rec_start[r];
        RtProb s = rt_prob_init();
        for (uint64_t v = v0; v < v1; ++v) {
            const uint32_t key = rt_probability_step(s, (uint32_t)(v - v0), ratios, p_of_quality, R, Q.var_pos[v], Q.var_u[v], Q.var_type[v], kind,
                                                     Q.snip_bytes + Q.snip_ptr[v], Q.snip_ptr[v + 1] - Q.snip_ptr[v], U.qual + q0, rec_len, rec_start);
            first = key < first ? key : first;
        }
        out_prob[c0 + j] = s.p;
    }
    for (int w = 32; w >= 1; w >>= 1) {          // the wavefront's lanes are together again here: the minimum over all 64
        const uint32_t other = (uint32_t)__shfl_xor((int)first, w);
        first = other < first ? other : first;
    }
    if (lane == 0) out_status[q] = rt_prob_status(first);
}

}  // namespace isocon
