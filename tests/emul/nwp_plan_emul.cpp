// Stand-alone driver of isocon_amd/csrc/nwp_plan.hpp (tests/test_nwp_plan.py; g++, also under -fsanitize=address,undefined).  Commands on
// stdin, one answer each on stdout:
//   plan <budget> <band_budget> <unbanded 0|1> <launch cap> <window 0|1> <hits>, then per hit "pair len_q len_t ed" (window: "... start cols"):
//       the plan of a path call over a store in which hit i has sequences 2 i (query) and 2 i + 1 (target).  Answer: "refused <status> <text>", or
//           "hits <n> unbanded <nu> w1 <n> w2 <n> w4 <n> lds <bytes> rev_total <runs>"
//           "cls ..." "cols ..." "units ..."         by hit
//           "ord ..." "rev_off ..."                  by position
//           "ulaunch <first position> <count> <units>"        per un-banded launch, then "toff ..." by position
//           "wave <W> <region cols> <lanes> <woff> <position> ..."        per wave
//           "blaunch <first wave> <count> <W> <units>"        per band launch
//           "stores <largest un-banded> <sum un-banded> <largest band> <sum band>"        in 16-byte units, then "end"
//       The properties of a plan are checked here (see check_plan): a violation is a message on stderr and exit status 3.
//   offsets <n_pairs> <hits>, then per hit "pair runs", then the hits' positions (ord), then n_pairs x extra
//       -> "ptr ..." (n_pairs + 1 values) and "foff ..." (by position)
//   cut <budget> <cap> <n>, then n x units        -> "launch <first> <count> <units>" per launch, "off ...", "stores <largest> <sum>", "end"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../isocon_amd/csrc/nwp_plan.hpp"

using namespace isocon;

#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(3); } } while (0)

template <class T>
static void print_row(const char *name, const std::vector<T> &v)
{
    printf("%s", name);
    for (const T &x : v) printf(" %lld", (long long)x);
    printf("\n");
}

// launches: non-empty, contiguous, within the cap and the budget; offsets: the running sums from 0 inside each
static void check_cut(const char *what, const BudgetCut &c, const std::vector<uint64_t> &units, uint64_t budget, size_t cap)
{
    const size_t n = units.size();
    REQUIRE(c.off.size() == n && !c.cut.empty() && c.cut[0] == 0 && (n ? c.cut.back() == n && c.cut.size() >= 2 : c.cut.size() == 1), "%s: boundaries", what);
    uint64_t most = 0, sum = 0;
    for (size_t l = 0; l + 1 < c.cut.size(); ++l) {
        REQUIRE(c.cut[l] < c.cut[l + 1] && c.cut[l + 1] - c.cut[l] <= cap, "%s: launch %zu holds %zu items", what, l, c.cut[l + 1] - c.cut[l]);
        uint64_t total = 0;
        for (size_t i = c.cut[l]; i < c.cut[l + 1]; ++i) {
            REQUIRE(c.off[i] == total, "%s: offset of item %zu", what, i);
            total += units[i];
        }
        REQUIRE(total * 16 <= budget, "%s: launch %zu needs %" PRIu64 " bytes", what, l, total * 16);
        most = std::max(most, total); sum += total;
    }
    REQUIRE(most == c.most && sum == c.sum, "%s: stores", what);
}

static void check_plan(const NwpPlan &P, const NwpHits &H, uint64_t budget, uint64_t band_budget, size_t cap)
{
    const size_t nh = H.pair.size(), nu = P.nu, nw = P.wcols.size();
    REQUIRE(P.cls.size() == nh && P.ncols.size() == nh && P.units_of.size() == nh && P.ord.size() == nh, "sizes by hit");
    REQUIRE(P.pq.size() == nh && P.pt.size() == nh && P.ped.size() == nh && P.pstart.size() == nh && P.pcols.size() == nh && P.rev_off.size() == nh, "sizes by position");
    // every hit at exactly one position; what is indexed by position follows ord; rev_off: the running sums of 2 ed + 1
    std::vector<int> seen(nh, 0);
    uint64_t rev = 0;
    std::vector<uint64_t> units(nu);
    for (size_t p = 0; p < nh; ++p) {
        const uint32_t i = P.ord[p];
        REQUIRE(i < nh && !seen[i]++, "position %zu: hit %u", p, i);
        REQUIRE(P.pq[p] == H.q[i] && P.pt[p] == H.t[i] && P.ped[p] == H.ed[i] && P.pcols[p] == P.ncols[i] && P.pstart[p] == (H.window() ? H.start[i] : 0), "position %zu: arrays", p);
        REQUIRE(P.rev_off[p] == rev, "position %zu: rev_off", p);
        rev += 2 * (uint64_t)H.ed[i] + 1;
        // the un-banded positions first, in the order of the list; the band positions by (class, columns, index)
        if (p < nu) {
            REQUIRE(P.cls[i] == 0 && (p == 0 || P.ord[p - 1] < i), "position %zu: un-banded order", p);
            units[p] = P.units_of[i];
        } else {
            REQUIRE(P.cls[i] != 0 && P.units_of[i] == 0, "position %zu: a band hit", p);
            if (p > nu) {
                const uint32_t h = P.ord[p - 1];
                REQUIRE(P.cls[h] < P.cls[i] || (P.cls[h] == P.cls[i] && (P.ncols[h] < P.ncols[i] || (P.ncols[h] == P.ncols[i] && h < i))), "position %zu: band order", p);
            }
        }
    }
    REQUIRE(rev == P.rev_total, "rev_total");
    check_cut("un-banded", P.unbanded, units, budget, cap);
    // waves: 1 to 64 lanes of one class, consecutive positions, the unused slots at the tail; the columns of the last lane, the longest
    REQUIRE(P.slots.size() == nw * 64 && P.wlanes.size() == nw && P.wcls.size() == nw && (nw != 0) == (nh > nu), "sizes by wave");
    size_t at = nu;
    std::vector<uint64_t> wunits(nw);
    for (size_t w = 0; w < nw; ++w) {
        const int32_t lanes = P.wlanes[w], W = P.wcls[w];
        REQUIRE(lanes >= 1 && lanes <= 64 && at + (size_t)lanes <= nh && (W == 1 || W == 2 || W == 4), "wave %zu: %d lanes of class %d", w, lanes, W);
        for (int32_t l = 0; l < 64; ++l) {
            const uint32_t p = P.slots[w * 64 + l];
            if (l >= lanes) { REQUIRE(p == 0xffffffffu, "wave %zu: slot %d is in use", w, l); continue; }
            REQUIRE(p == at && p < nh && P.cls[P.ord[p]] == W && P.pcols[p] <= P.pcols[at + (lanes - 1 - l)], "wave %zu: slot %d", w, l);
            ++at;
        }
        REQUIRE(P.wcols[w] == ((P.pcols[at - 1] + 31) / 32) * 32, "wave %zu: columns", w);
        wunits[w] = (uint64_t)P.wcols[w] * (uint64_t)W * (uint64_t)lanes;
    }
    REQUIRE(at == nh, "the waves hold %zu positions of %zu", at, nh);
    check_cut("band", P.band, wunits, band_budget, cap);
    for (size_t l = 0; l + 1 < P.band.cut.size(); ++l)
        for (size_t w = P.band.cut[l]; w < P.band.cut[l + 1]; ++w) REQUIRE(P.wcls[w] == P.wcls[P.band.cut[l]], "band launch %zu: two classes", l);
}

int main()
{
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "plan")) {
            uint64_t budget = 0, band_budget = 0;
            int unbanded = 0, window = 0;
            size_t cap = 0, nh = 0;
            REQUIRE(scanf("%" SCNu64 " %" SCNu64 " %d %zu %d %zu", &budget, &band_budget, &unbanded, &cap, &window, &nh) == 6, "plan: header");
            std::vector<int32_t> lens(2 * nh);
            NwpHits H;
            for (size_t i = 0; i < nh; ++i) {
                uint64_t pair = 0;
                int32_t ed = 0, start = 0, cols = 0;
                REQUIRE(scanf("%" SCNu64 " %d %d %d", &pair, &lens[2 * i], &lens[2 * i + 1], &ed) == 4 && (!window || scanf("%d %d", &start, &cols) == 2), "plan: hit %zu", i);
                H.pair.push_back(pair); H.q.push_back((uint32_t)(2 * i)); H.t.push_back((uint32_t)(2 * i + 1)); H.ed.push_back(ed);
                if (window) { H.start.push_back(start); H.cols.push_back(cols); }
            }
            NwpPlan P;
            std::string error;
            const int rc = nwp_plan(lens, H, budget, band_budget, unbanded != 0, P, error, cap);
            if (rc) { printf("refused %d %s\n", rc, error.c_str()); continue; }
            check_plan(P, H, budget, band_budget, cap);
            printf("hits %zu unbanded %zu w1 %.0f w2 %.0f w4 %.0f lds %zu rev_total %" PRIu64 "\n", nh, P.nu, P.per_class[1], P.per_class[2], P.per_class[4], P.lds, P.rev_total);
            print_row("cls", P.cls); print_row("cols", P.ncols); print_row("units", P.units_of);
            print_row("ord", P.ord); print_row("rev_off", P.rev_off);
            for (size_t l = 0; l + 1 < P.unbanded.cut.size(); ++l) {
                const size_t a = P.unbanded.cut[l], b = P.unbanded.cut[l + 1];
                printf("ulaunch %zu %zu %" PRIu64 "\n", a, b - a, P.unbanded.off[b - 1] + P.units_of[P.ord[b - 1]]);
            }
            print_row("toff", P.unbanded.off);
            for (size_t w = 0; w < P.wcols.size(); ++w) {
                printf("wave %d %d %d %" PRIu64, P.wcls[w], P.wcols[w], P.wlanes[w], P.band.off[w]);
                for (int32_t l = 0; l < P.wlanes[w]; ++l) printf(" %u", P.slots[w * 64 + l]);
                printf("\n");
            }
            for (size_t l = 0; l + 1 < P.band.cut.size(); ++l) {
                const size_t a = P.band.cut[l], b = P.band.cut[l + 1];
                printf("blaunch %zu %zu %d %" PRIu64 "\n", a, b - a, P.wcls[a], P.band.off[b - 1] + (uint64_t)P.wcols[b - 1] * P.wcls[b - 1] * P.wlanes[b - 1]);
            }
            printf("stores %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\nend\n", P.unbanded.most, P.unbanded.sum, P.band.most, P.band.sum);
        } else if (!strcmp(cmd, "offsets")) {
            uint64_t n_pairs = 0;
            size_t nh = 0;
            REQUIRE(scanf("%" SCNu64 " %zu", &n_pairs, &nh) == 2, "offsets: header");
            NwpHits H;
            std::vector<int32_t> runs(nh);
            std::vector<uint32_t> ord(nh);
            std::vector<int> extra(n_pairs);
            for (size_t i = 0; i < nh; ++i) {
                uint64_t pair = 0;
                REQUIRE(scanf("%" SCNu64 " %d", &pair, &runs[i]) == 2 && pair < n_pairs, "offsets: hit %zu", i);
                H.pair.push_back(pair);
            }
            for (uint32_t &p : ord) REQUIRE(scanf("%u", &p) == 1 && p < nh, "offsets: ord");
            for (int &x : extra) REQUIRE(scanf("%d", &x) == 1, "offsets: extra");
            std::vector<uint64_t> ptr(n_pairs + 1), foff;
            nwp_forward_offsets(H, ord, runs, n_pairs, [&](uint64_t p) -> uint64_t { return (uint64_t)extra[p]; }, ptr.data(), foff);
            REQUIRE(foff.size() == nh, "offsets: foff");
            print_row("ptr", ptr); print_row("foff", foff);
        } else if (!strcmp(cmd, "cut")) {
            uint64_t budget = 0;
            size_t cap = 0, n = 0;
            REQUIRE(scanf("%" SCNu64 " %zu %zu", &budget, &cap, &n) == 3, "cut: header");
            std::vector<uint64_t> units(n);
            for (uint64_t &u : units) REQUIRE(scanf("%" SCNu64, &u) == 1, "cut: units");
            const BudgetCut c = cap ? budget_cut(units.data(), n, budget, cap) : budget_cut(units.data(), n, budget);          // cap 0: the default
            check_cut("cut", c, units, budget, cap ? cap : (size_t)1 << 20);
            for (size_t l = 0; l + 1 < c.cut.size(); ++l) printf("launch %zu %zu %" PRIu64 "\n", c.cut[l], c.cut[l + 1] - c.cut[l], c.off[c.cut[l + 1] - 1] + units[c.cut[l + 1] - 1]);
            print_row("off", c.off);
            printf("stores %" PRIu64 " %" PRIu64 "\nend\n", c.most, c.sum);
        } else REQUIRE(false, "unknown command %s", cmd);
    }
    return 0;
}
