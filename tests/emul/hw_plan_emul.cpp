// Stand-alone driver of isocon_amd/csrc/hw_plan.hpp (tests/test_hw_plan.py; g++, also under -fsanitize=address,undefined).  Commands on
// stdin, one answer each on stdout:
//   locate <nseq> <npairs>, then nseq lengths, then npairs x "q t k": the LOCATE-shaped cut of the pairs that need a kernel
//   finish <nseq> <npairs>, then npairs x "q k":                     the FINISH-shaped cut of all pairs (hits)
//       answer: one line "tile <W> <query> <pair> ..." per tile in class order, then "end".  The properties of a cut are checked here (each
//       listed pair in exactly one lane, 64 lanes per tile with empty ones at its tail only, one query per tile, the common window of a
//       tile within its class): a violation is a message on stderr and exit status 3.
//   words <rows>                                  -> "<hwt_words> <hwt_class>"
//   cap <W>                                       -> "<hw_finish_grid_cap> <hw_finish_lds>"
//   store <W> <trace_cols>                        -> "<hw_finish_store_bytes>"
//   grid <n_tiles> <W> <trace_cols> <free_bytes>  -> "<hw_finish_grid>"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../isocon_amd/csrc/hw_plan.hpp"

using namespace isocon;

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(3); } } while (0)

// rows(lanes) = diagonals of the common window of a tile's lanes
template <class Rule, class Rows>
static void cut_and_print(const std::vector<uint32_t> &idx, const std::vector<uint32_t> &q, uint32_t nseq, const Rule &rule, Rows rows)
{
    HwTiles tiles;
    hw_build_tiles(idx, q.data(), nseq, rule, tiles);
    std::vector<int> seen(q.size(), 0);
    for (int c = 0; c < 4; ++c) {
        const std::vector<uint32_t> &tq = tiles.tile_q[c], &lp = tiles.lane_pair[c];
        REQUIRE(lp.size() == 64 * tq.size(), "class %d: %zu lanes for %zu tiles", c, lp.size(), tq.size());
        for (size_t tile = 0; tile < tq.size(); ++tile) {
            std::vector<uint32_t> lanes;
            for (size_t l = 0; l < 64; ++l) {
                const uint32_t p = lp[tile * 64 + l];
                if (p == 0xffffffffu) continue;
                REQUIRE(lanes.size() == l, "class %d tile %zu: an empty lane in front of lane %zu", c, tile, l);
                REQUIRE(p < q.size() && q[p] == tq[tile], "class %d tile %zu lane %zu: pair %u is not one of query %u", c, tile, l, p, tq[tile]);
                ++seen[p];
                lanes.push_back(p);
            }
            REQUIRE(!lanes.empty(), "class %d tile %zu is empty", c, tile);
            REQUIRE(rows(lanes) <= 64 << c, "class %d tile %zu: common window of %d diagonals", c, tile, (int)rows(lanes));
            printf("tile %d %u", 1 << c, tq[tile]);
            for (uint32_t p : lanes) printf(" %u", p);
            printf("\n");
        }
    }
    for (uint32_t p : idx) { REQUIRE(seen[p] == 1, "pair %u sits in %d lanes", p, seen[p]); seen[p] = 0; }
    for (size_t p = 0; p < seen.size(); ++p) REQUIRE(seen[p] == 0, "pair %zu needs no kernel and sits in a lane", p);
    printf("end\n");
}

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "locate") || !strcmp(cmd, "finish")) {
            const bool locate = cmd[0] == 'l';
            uint32_t nseq = 0, npairs = 0;
            REQUIRE(scanf("%u %u", &nseq, &npairs) == 2, "%s: counts", cmd);
            std::vector<int32_t> lens(nseq, 0);
            std::vector<uint32_t> q(npairs), t(npairs, 0), idx;
            std::vector<int32_t> k(npairs);
            if (locate) for (int32_t &x : lens) REQUIRE(scanf("%d", &x) == 1, "locate: lengths");
            for (uint32_t p = 0; p < npairs; ++p) {
                REQUIRE((locate ? scanf("%u %u %d", &q[p], &t[p], &k[p]) == 3 : scanf("%u %d", &q[p], &k[p]) == 2) && q[p] < nseq && t[p] < nseq && k[p] >= 0, "%s: pair %u", cmd, p);
                // (the rule of hw_pairs_host_tiles: distance >= len(q) - len(t) > k, or an empty sequence, needs no kernel)
                if (!locate || !(lens[t[p]] - lens[q[p]] < -k[p] || lens[q[p]] == 0 || lens[t[p]] == 0)) idx.push_back(p);
            }
            if (locate) {
                const HwLocateCut rule{lens.data(), q.data(), t.data(), k.data()};
                cut_and_print(idx, q, nseq, rule, [&](const std::vector<uint32_t> &lanes) {
                    int32_t dmax = -(1 << 30), kmax = 0;
                    for (uint32_t p : lanes) { dmax = std::max(dmax, rule.delta(p)); kmax = std::max(kmax, k[p]); }
                    return hw_locate_rows(dmax, kmax);
                });
            } else {
                cut_and_print(idx, q, nseq, HwFinishCut{k.data()}, [&](const std::vector<uint32_t> &lanes) {
                    int32_t kmax = 0;
                    for (uint32_t p : lanes) kmax = std::max(kmax, k[p]);
                    return 2 * kmax + 1;
                });
            }
        } else if (!strcmp(cmd, "words")) {
            int32_t rows = 0;
            REQUIRE(scanf("%d", &rows) == 1, "words: rows");
            printf("%d %u\n", hwt_words(rows), hwt_class(hwt_words(rows)));
        } else if (!strcmp(cmd, "cap")) {
            int W = 0;
            REQUIRE(scanf("%d", &W) == 1, "cap: W");
            printf("%u %zu\n", hw_finish_grid_cap(W), hw_finish_lds(W));
        } else if (!strcmp(cmd, "store")) {
            int W = 0;
            uint32_t cols = 0;
            REQUIRE(scanf("%d %u", &W, &cols) == 2, "store: W, trace_cols");
            printf("%" PRIu64 "\n", hw_finish_store_bytes(W, cols));
        } else if (!strcmp(cmd, "grid")) {
            int W = 0;
            uint32_t n_tiles = 0, cols = 0;
            uint64_t free_bytes = 0;
            REQUIRE(scanf("%u %d %u %" SCNu64, &n_tiles, &W, &cols, &free_bytes) == 4, "grid: n_tiles, W, trace_cols, free_bytes");
            printf("%u\n", hw_finish_grid(n_tiles, W, cols, free_bytes));
        } else REQUIRE(false, "unknown command %s", cmd);
    }
    return 0;
}
