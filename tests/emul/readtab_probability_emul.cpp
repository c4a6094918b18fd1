// CPU driver of rt_probability_step (isocon_amd/csrc/readtab_core.hpp) in the shape of k_rt_probability (readtab.hpp): 64 emulated lanes per
// query, every lane walks its rows j = lane, lane + 64, ... with (alive, p) kept over the variant loop, the lanes' smallest event keys
// meet in an xor butterfly and lane 0 writes the status word.  A program of its own (tests/test_readtab_probability_core.py builds it
// with g++ -O2 -ffp-contract=off and a second time under -fsanitize=undefined,address): it reads a case file and writes a result file.
//   case file   18 arrays, each a uint64 byte count followed by its bytes: candidate rows, read rows, row_ptr (u64), first_row (u32),
//               qual (u8), qual_ptr (u64), rec_start (u32), q_table (u32), q_kind (u8), var_ptr (u64), var_pos (u32, wrapped into
//               [0, ref_len)), var_u (i32), var_type (u8), snip_ptr (u64), snip_bytes (u8), q_ratios (f64, 3 per query), p_of_quality
//               (f64, 94), prob_ptr (u64)
//   result file prob_ptr[n_queries] doubles (slots beyond a table's rows stay 0.0), then n_queries status words (u32)
// The tables come from the emulated k_rt_build / k_rt_read_prefix of readtab_quality_emul.cpp (included).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "readtab_quality_emul.cpp"

namespace {

std::vector<uint8_t> read_array(FILE *f)
{
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) { fprintf(stderr, "case file: truncated\n"); exit(2); }
    std::vector<uint8_t> a((size_t)n);
    if (n && fread(a.data(), 1, (size_t)n, f) != n) { fprintf(stderr, "case file: truncated\n"); exit(2); }
    return a;
}

template <class T>
std::vector<T> as(const std::vector<uint8_t> &raw)
{
    std::vector<T> out(raw.size() / sizeof(T));
    if (!out.empty()) memcpy(out.data(), raw.data(), out.size() * sizeof(T));
    return out;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s case-file result-file\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const std::vector<uint8_t> ref = read_array(f), read = read_array(f);
    const auto row_ptr = as<uint64_t>(read_array(f));
    const auto first_row = as<uint32_t>(read_array(f));
    const std::vector<uint8_t> qual = read_array(f);
    const auto qual_ptr = as<uint64_t>(read_array(f));
    const auto rec_start = as<uint32_t>(read_array(f));
    const auto q_table = as<uint32_t>(read_array(f));
    const std::vector<uint8_t> q_kind = read_array(f);
    const auto var_ptr = as<uint64_t>(read_array(f));
    const auto var_pos = as<uint32_t>(read_array(f));
    const auto var_u = as<int32_t>(read_array(f));
    const std::vector<uint8_t> var_type = read_array(f);
    const auto snip_ptr = as<uint64_t>(read_array(f));
    const std::vector<uint8_t> snip_bytes = read_array(f);
    const auto q_ratios = as<double>(read_array(f));
    const auto p_of_quality = as<double>(read_array(f));
    const auto prob_ptr = as<uint64_t>(read_array(f));
    fclose(f);
    const uint32_t n_rows = (uint32_t)row_ptr.size() - 1, n_queries = (uint32_t)q_table.size();
    if (p_of_quality.size() != 94 || q_ratios.size() != (size_t)n_queries * 3 || prob_ptr.size() != (size_t)n_queries + 1 || qual_ptr.size() != (size_t)n_rows + 1 ||
        rec_start.size() != n_rows || var_ptr.size() != (size_t)n_queries + 1) {
        fprintf(stderr, "case file: array sizes do not fit\n");
        return 2;
    }

    // the tables (k_rt_build, k_rt_read_prefix)
    std::vector<uint64_t> blk_ptr((size_t)n_rows + 1, 0);
    for (uint32_t r = 0; r < n_rows; ++r) blk_ptr[r + 1] = blk_ptr[r] + (row_ptr[r + 1] - row_ptr[r] + 63) / 64;
    const size_t n_blk = (size_t)blk_ptr[n_rows];
    std::vector<uint64_t> nob(n_blk), diff(n_blk), rgap(n_blk);
    std::vector<uint32_t> pre(n_blk), rpre(n_blk), errors((size_t)n_rows * 4);
    if (rt_emul_build(ref.data(), read.data(), row_ptr.data(), blk_ptr.data(), n_rows, nob.data(), diff.data(), pre.data(), errors.data())) {
        fprintf(stderr, "a row holds a byte outside ACGT-\n");
        return 2;
    }
    rt_emul_read_prefix(read.data(), row_ptr.data(), blk_ptr.data(), n_rows, rgap.data(), rpre.data());

    // k_rt_probability
    std::vector<double> out_prob((size_t)prob_ptr[n_queries], 0.0);
    std::vector<uint32_t> out_status(n_queries, 0xABABABABu);
    for (uint32_t q = 0; q < n_queries; ++q) {
        const uint32_t k = q_table[q], r0 = first_row[k], nr = first_row[k + 1] - r0;
        const uint64_t v0 = var_ptr[q], v1 = var_ptr[q + 1], c0 = prob_ptr[q];
        const double *ratios = q_ratios.data() + (size_t)q * 3;
        uint32_t first[64];
        for (int lane = 0; lane < 64; ++lane) {
            first[lane] = RT_P_NO_EVENT;
            for (uint32_t j = (uint32_t)lane; j < nr; j += 64) {
                const uint64_t r = (uint64_t)r0 + j, off = row_ptr[r], blk0 = blk_ptr[r], q0 = qual_ptr[r];
                const RtRow R{nob.data() + blk0, diff.data() + blk0, pre.data() + blk0, read.data() + off, (uint32_t)(blk_ptr[r + 1] - blk0), (int64_t)(row_ptr[r + 1] - off),
                              rgap.data() + blk0, rpre.data() + blk0};
                RtProb s = rt_prob_init();
                for (uint64_t v = v0; v < v1; ++v) {
                    const uint32_t key = rt_probability_step(s, (uint32_t)(v - v0), ratios, p_of_quality.data(), R, var_pos[v], var_u[v], var_type[v], q_kind[q],
                                                             snip_bytes.data() + snip_ptr[v], snip_ptr[v + 1] - snip_ptr[v], qual.data() + q0, (int64_t)(qual_ptr[r + 1] - q0),
                                                             rec_start[r]);
                    first[lane] = key < first[lane] ? key : first[lane];
                }
                out_prob[c0 + j] = s.p;
            }
        }
        for (int w = 32; w >= 1; w >>= 1) {          // the xor butterfly: every lane takes the smaller of its own and its partner's
            uint32_t next[64];
            for (int lane = 0; lane < 64; ++lane) next[lane] = first[lane ^ w] < first[lane] ? first[lane ^ w] : first[lane];
            memcpy(first, next, sizeof(first));
        }
        out_status[q] = rt_prob_status(first[0]);
    }

    FILE *g = fopen(argv[2], "wb");
    if (!g) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    if (!out_prob.empty()) fwrite(out_prob.data(), 8, out_prob.size(), g);
    if (!out_status.empty()) fwrite(out_status.data(), 4, out_status.size(), g);
    return fclose(g) == 0 ? 0 : 2;
}
