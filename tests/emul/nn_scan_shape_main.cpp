// The launch shapes isocon_amd/csrc/nn_scan_shape.hpp chooses, printed for tests/test_nn_scan_shape.py (a program of its own: g++, plain and
// with -fsanitize=undefined,address).  stdin: one maxlen per line.  argv: --pad N adds the shape of the nn_lds_pad experiment.
// stdout, one line per maxlen:
//   maxlen ring4 ring8 ring12 ring16 fits64 | four shapes "waves lds raise" for (preferred 4, 8) x (64-row, 32-row) | tile kernel, its LDS
//   | for W = 2 .. 8: lds of the 64 W-row form, fits with 12 waves, fits with 16 waves [| padded shape]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../isocon_amd/csrc/nn_scan_shape.hpp"

using namespace isocon;

static void print_shape(const NNRefillShape &s) { printf(" %d %zu %d", s.waves, s.lds, (int)s.raise_limit); }

int main(int argc, char **argv)
{
    int pad = -1;
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--pad")) pad = atoi(argv[i + 1]);
    long v;
    while (scanf("%ld", &v) == 1) {
        const int32_t maxlen = (int32_t)v;
        printf("%d %zu %zu %zu %zu %d", maxlen, nn_ring_bytes(4), nn_ring_bytes(8), nn_ring_bytes(12), nn_ring_bytes(16), (int)nn_refill64_fits(maxlen));
        for (int preferred = 4; preferred <= 8; preferred += 4)
            for (int half = 0; half < 2; ++half) print_shape(nn_refill_shape(maxlen, preferred, half != 0));
        printf(" %d %zu", (int)nn_tile_scan(maxlen), nn_tile_scan_lds(maxlen));
        for (int W = 2; W <= 8; ++W) printf(" %zu %d %d", nn_refill_lds(maxlen, 64 * W), (int)nn_refill_fits(maxlen, 64 * W, 12), (int)nn_refill_fits(maxlen, 64 * W, 16));
        if (pad >= 0) print_shape(nn_refill_shape_padded(maxlen, pad));
        printf("\n");
    }
    return 0;
}
