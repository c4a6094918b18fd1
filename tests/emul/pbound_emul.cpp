// CPU emulator of k_pvalue_bound (isocon_amd/csrc/pbound.hpp): the lane math of pbound_core.hpp, one test after the other.
//     pbound_emul <case file> <result file>
// case file: n pairs (m_sum, y_sum) of doubles.  result file: n doubles (the bound; 0.0 where not certified), n bytes (certified), then for
// diagnosis n doubles err_total (the bound on the error of E, absolute) and n doubles: the distance of the discarded bits from the halfway
// pattern in ulps of the result (not meaningful where the result is 0.0).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../isocon_amd/csrc/pbound_core.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint64_t> in;
    uint64_t pair[2];
    while (fread(pair, 8, 2, f) == 2) { in.push_back(pair[0]); in.push_back(pair[1]); }
    fclose(f);
    const size_t n = in.size() / 2;
    std::vector<uint64_t> bound(n);
    std::vector<uint8_t> certified(n);
    std::vector<double> err(n), dist(n);
    for (size_t i = 0; i < n; ++i) {
        isocon::PbDiag d;
        bound[i] = isocon::pb_eval(in[2 * i], in[2 * i + 1], &certified[i], &d);
        err[i] = std::ldexp((double)d.err_total, -256);
        double x = 0.0;
        for (int l = isocon::PB_NL - 1; l >= 0; --l) x = x * 4294967296.0 + (double)d.dist.w[l];
        dist[i] = std::ldexp(x, -d.p);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    bool ok = fwrite(bound.data(), 8, n, f) == n && fwrite(certified.data(), 1, n, f) == n && fwrite(err.data(), 8, n, f) == n && fwrite(dist.data(), 8, n, f) == n;
    ok = fclose(f) == 0 && ok;
    return ok ? 0 : 1;
}
