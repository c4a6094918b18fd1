// CPU run of the lane-per-pair un-banded infix kernel (isocon_amd/csrc/hw_rows.hpp k_hwl_rows) on the SAME lane-level math header
// (hw_rows_core.hpp): one lane = one pair, the query in W = 1, 2 or 4 words -- the smallest that holds it, or argv[1] --, the target
// taken 64 columns at a time as the kernel streams it.  A program of its own (tests/test_hw_locations_wide_core.py builds it plain and
// under sanitizers); protocol: hw_wide_emul.hpp.
#include <cstdlib>
#include "hw_wide_emul.hpp"

template <int W>
static void rows_run(const Planes &Q, const Planes &T, int32_t m, int32_t n, int32_t h, bool fill, HwrCount &C, std::vector<int32_t> &listed)
{
    HwrLane<W> L;
    hwr_init<W>(L, [&](int w) { return w < (int)Q.lo.size() ? Q.lo[w] : 0; }, [&](int w) { return w < (int)Q.hi.size() ? Q.hi[w] : 0; }, m);
    for (int32_t j0 = 0; j0 < n; j0 += 64) {
        uint64_t tl = T.lo[j0 >> 6], th = T.hi[j0 >> 6];
        for (int32_t b = 0; b < 64 && j0 + b < n; ++b) {
            hwr_step<W>(L, (int32_t)(tl & 1u) | ((int32_t)(th & 1u) << 1));
            if (!fill) hwr_count_add(C, L.score, j0 + b);
            else if (L.score == h) listed.push_back(j0 + b);
            tl >>= 1; th >>= 1;
        }
    }
}

int main(int argc, char **argv)
{
    const int forced = argc > 1 ? atoi(argv[1]) : 0;
    return serve([&](const Planes &Q, const Planes &T, int32_t m, int32_t n, int32_t h, bool fill, HwrCount &C, std::vector<int32_t> &listed) {
        int w = hwr_words(m);
        if (forced > w && w) w = forced;
        if (w == 1) rows_run<1>(Q, T, m, n, h, fill, C, listed);
        else if (w == 2) rows_run<2>(Q, T, m, n, h, fill, C, listed);
        else if (w == 4) rows_run<4>(Q, T, m, n, h, fill, C, listed);
        else { fprintf(stderr, "a query of %d rows does not fit 4 words\n", m); exit(2); }
    });
}
