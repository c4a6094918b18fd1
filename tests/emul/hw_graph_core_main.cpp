// Stand-alone driver of isocon_amd/csrc/hw_graph_core.hpp (tests/test_hw_graph_core.py; g++, also under -fsanitize=undefined,address).
//   pairs  <window> <depth> <n> <len_0> ... <len_{n-1}>
//       line 1: n_pairs; then one line per entry "i cd cu", followed by one line per slot "i r t reverse_slot slot_of(i, t)" in
//       slot order, where reverse_slot = the slot of i in the list of t (from t's own counts)
//   adjust <T> <max_ed> <rows>  then per row: ed start end lead trail len_t
//       one value per line: hwg_edge_value
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../isocon_amd/csrc/hw_graph_core.hpp"

using namespace isocon;

int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "pairs")) {
        const int32_t window = (int32_t)strtol(argv[2], nullptr, 10);
        const uint64_t depth = strtoull(argv[3], nullptr, 10);
        const uint32_t n = (uint32_t)strtoul(argv[4], nullptr, 10);
        if ((int)n != argc - 5) { fprintf(stderr, "expected %u lengths\n", n); return 2; }
        std::vector<int32_t> lens(n);
        for (uint32_t i = 0; i < n; ++i) lens[i] = (int32_t)strtol(argv[5 + i], nullptr, 10);
        const uint32_t jmax = hwg_jmax(depth, n);
        std::vector<uint32_t> cd(n), cu(n);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; ++i) { hwg_counts(lens.data(), n, i, window, jmax, cd[i], cu[i]); total += cd[i] + cu[i]; }
        printf("%" PRIu64 "\n", total);
        for (uint32_t i = 0; i < n; ++i) {
            printf("%u %u %u\n", i, cd[i], cu[i]);
            for (uint32_t r = 0; r < cd[i] + cu[i]; ++r) {
                const uint32_t t = hwg_slot_target(i, cd[i], cu[i], r);
                if (t >= n) { fprintf(stderr, "entry %u slot %u: target %u out of range\n", i, r, t); return 3; }
                printf("%u %u %u %u %u\n", i, r, t, hwg_slot_of(t, cd[t], cu[t], i), hwg_slot_of(i, cd[i], cu[i], t));
            }
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "adjust")) {
        const int32_t T = (int32_t)strtol(argv[2], nullptr, 10), max_ed = (int32_t)strtol(argv[3], nullptr, 10);
        const long rows = strtol(argv[4], nullptr, 10);
        for (long p = 0; p < rows; ++p) {
            int32_t row[5], len_t;
            if (scanf("%d %d %d %d %d %d", &row[0], &row[1], &row[2], &row[3], &row[4], &len_t) != 6) return 2;
            printf("%d\n", hwg_edge_value(row, len_t, T, max_ed));
        }
        return 0;
    }
    fprintf(stderr, "usage: pairs <window> <depth> <n> <lens...> | adjust <T> <max_ed> <rows>\n");
    return 2;
}
