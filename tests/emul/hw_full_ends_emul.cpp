// CPU emulation of one wavefront (one pair) of the wavefront-per-pair ends kernel (isocon_amd/csrc/hw_rows.hpp k_hwl_wave: hwf_run of
// hw_full.hpp in mode ENDS): 64 lanes in lock step on the SAME lane-level math header (hw_full_core.hpp), the lane that owns the
// query's last row counts, then lists.  A program of its own (tests/test_hw_locations_wide_core.py builds it plain and under
// sanitizers); protocol: hw_wide_emul.hpp.
#include "hw_wide_emul.hpp"

int main()
{
    return serve([](const Planes &Q, const Planes &T, int32_t m, int32_t n, int32_t h, bool fill, HwrCount &C, std::vector<int32_t> &listed) {
        int32_t col;
        wave_run<HWF_ENDS>(Q, m, n, h, [&](int32_t c) { return T.base(c); }, [&](int32_t score, int32_t c) {
            if (!fill) hwr_count_add(C, score, c);
            else if (score == h) listed.push_back(c);
        }, col);
    });
}
