// CPU driver of the task cutting of isocon_amd/csrc/nn2_depth_core.hpp (tests/test_nn2set_tasks_core.py; a program of its own, so
// that it also runs under sanitizers): nn2_cut_list, the routine the test entry isocon_nn2_block_reject cuts its pair list with, and
// through it nn2_cut_tasks, which the listing kernel of nn2_depth.hpp calls on a read's run.
//
// stdin: the number of pairs, then per pair "read tested" (tested: 0 / 1).  stdout: one line "read first pairs" per task, in the
// order they were cut, then "tasks N" with the routine's return value.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../isocon_amd/csrc/nn2_depth_core.hpp"

using namespace isocon;

int main()
{
    unsigned long long n = 0;
    if (scanf("%llu", &n) != 1) return 2;
    std::vector<uint32_t> read(n);
    std::vector<int> tested(n);
    for (unsigned long long p = 0; p < n; ++p)
        if (scanf("%u %d", &read[p], &tested[p]) != 2) return 2;
    const unsigned long long n_tasks = nn2_cut_list(read.data(), n, [&](unsigned long long p) { return tested[p] != 0; },
                                                    [](uint32_t x, unsigned long long first, uint32_t pairs) { printf("%u %llu %u\n", x, first, pairs); });
    printf("tasks %llu\n", n_tasks);
    return 0;
}
