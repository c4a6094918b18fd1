// CPU: the two sources of the fast path's match vectors in lane_pair_distance (isocon_amd/csrc/ed_lanes_core.hpp) against each other and
// against a textbook DP.  EqFromTable (what k_ed_lanes runs: four masks per block in a slot of the lane's own, one 16-byte read per column,
// requested a few columns ahead) must hand out, column for column, the 64 bits EqFromPlanes builds from the plane registers, and both
// distances must be the DP's.  The table is a plain array with the layout the kernel has in LDS; every pair runs as another (wave, lane) of
// a workgroup, the array is filled with a canary first and everything outside the lane's four records must still hold it afterwards.
//
// A program of its own (tests/test_lanes_eq_table_core.py builds it plain and with -fsanitize=address,undefined):
//   lanes_eq_table_emul [quick]      prints "ok <pairs> <fast columns> <blocks whose window passes the pattern's end> <within-threshold pairs>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../isocon_amd/csrc/ed_lanes_core.hpp"

using namespace isocon;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static uint32_t rnd(uint32_t n) { return rnd() % n; }

static void pack(const std::string &s, std::vector<uint64_t> &lo, std::vector<uint64_t> &hi)
{
    const int nc = ((int)s.size() + 63) / 64 + 2;
    lo.assign(nc, 0); hi.assign(nc, 0);
    for (size_t i = 0; i < s.size(); ++i) {
        const int code = s[i] == 'A' ? 0 : s[i] == 'C' ? 1 : s[i] == 'G' ? 2 : 3;
        if (code & 1) lo[i >> 6] |= (uint64_t)1 << (i & 63);
        if (code & 2) hi[i >> 6] |= (uint64_t)1 << (i & 63);
    }
}

static int dp(const std::string &x, const std::string &y)
{
    const int m = (int)x.size(), n = (int)y.size();
    std::vector<int> prev(m + 1), cur(m + 1);
    for (int i = 0; i <= m; ++i) prev[i] = i;
    for (int j = 1; j <= n; ++j) {
        cur[0] = j;
        for (int i = 1; i <= m; ++i) cur[i] = std::min(std::min(prev[i] + 1, cur[i - 1] + 1), prev[i - 1] + (x[i - 1] != y[j - 1]));
        prev.swap(cur);
    }
    return prev[m];
}

// what the fast path saw: per block the text words and whether the 96 positions pass the pattern's end, per column the 64 bits of Eq
struct Log {
    std::vector<uint64_t> eq;
    std::vector<uint32_t> text;
    uint64_t base_seen[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};     // [column parity][base]
};

template <class Base>
struct Recorded : Base {
    Log *log;
    template <class... A> Recorded(Log *l, A... a) : Base(a...), log(l) {}
    void block(uint32_t L0, uint32_t L1, uint32_t L2, uint32_t H0, uint32_t H1, uint32_t H2, uint32_t wl, uint32_t wh)
    {
        Base::block(L0, L1, L2, H0, H1, H2, wl, wh);
        log->text.push_back(wl); log->text.push_back(wh);
        for (int jj = 0; jj < 32; ++jj) ++log->base_seen[jj & 1][((wl >> jj) & 1u) | (((wh >> jj) & 1u) << 1)];
    }
    void column(int jj, uint32_t &e0, uint32_t &e1)
    {
        Base::column(jj, e0, e1);
        log->eq.push_back(((uint64_t)e1 << 32) | e0);
    }
};

static const uint32_t CANARY = 0xC0FFEE11u;
static std::vector<eq_rec_t> table(4 * EQ_TABLE_RECS);
static uint64_t n_pairs = 0, n_fast_columns = 0, n_end_blocks = 0, n_within = 0;
static uint64_t base_seen[2][4];

static void fail(const char *what, const std::string &x, const std::string &y, int k, long a, long b)
{
    std::printf("FAIL %s: m=%zu n=%zu k=%d got %ld want %ld\nx=%s\ny=%s\n", what, x.size(), y.size(), k, a, b, x.c_str(), y.c_str());
    std::exit(1);
}

static void one_pair(const std::string &x, const std::string &y, int k)
{
    const int m = (int)x.size(), n = (int)y.size();
    const int d = m - n, ad = d < 0 ? -d : d;
    if (k < 0 || ad > k || m == 0 || n == 0) return;        // the caller's cases (k_ed_lanes decides them before the lane runs)
    std::vector<uint64_t> xl, xh, yl, yh;
    pack(x, xl, xh);
    pack(y, yl, yh);
    auto f = [](const std::vector<uint64_t> &v) { return [&v](int32_t ci) -> uint64_t { return ci >= 0 && ci < (int)v.size() ? v[ci] : 0; }; };
    auto any = [](bool b) { return b; };
    const int want_d = dp(x, y), want = want_d <= k ? want_d : -1;
    // the present nine-argument call, the register form by name, and the table form as another lane of the workgroup each time
    const int32_t r9 = lane_pair_distance(f(xl), f(xh), f(yl), f(yh), m, n, k, true, any);
    Log lp, lt;
    const int32_t rp = lane_pair_distance(f(xl), f(xh), f(yl), f(yh), m, n, k, true, any, Recorded<EqFromPlanes>(&lp));
    const uint32_t wave = (uint32_t)(n_pairs & 3), lane = (uint32_t)((n_pairs >> 2) * 37 % EQ_TABLE_LANES);
    for (eq_rec_t &r : table) r = eq_rec_t{CANARY, CANARY, CANARY, CANARY};
    const int32_t rt = lane_pair_distance(f(xl), f(xh), f(yl), f(yh), m, n, k, true, any, Recorded<EqFromTable>(&lt, table.data(), wave, lane));
    if (r9 != want) fail("nine-argument call against the DP", x, y, k, r9, want);
    if (rp != want) fail("register form against the DP", x, y, k, rp, want);
    if (rt != want) fail("table form against the DP", x, y, k, rt, want);
    if (lp.text != lt.text) fail("fast-path blocks", x, y, k, (long)lt.text.size(), (long)lp.text.size());
    if (lp.eq.size() != lt.eq.size() || lp.eq.size() != 16 * lp.text.size()) fail("fast-path columns", x, y, k, (long)lt.eq.size(), (long)lp.eq.size());
    for (size_t c = 0; c < lp.eq.size(); ++c)
        if (lp.eq[c] != lt.eq[c]) fail("Eq of a fast-path column (got: its index, want: the differing bits)", x, y, k, (long)c, (long)(lp.eq[c] ^ lt.eq[c]));
    // nothing outside the lane's four records was written
    for (uint32_t i = 0; i < table.size(); ++i) {
        const bool own = (i & ~(3u * EQ_TABLE_LANES)) == (wave * EQ_TABLE_RECS | lane);
        if (!own && (table[i][0] != CANARY || table[i][1] != CANARY || table[i][2] != CANARY || table[i][3] != CANARY))
            fail("a record of another lane was written", x, y, k, (long)i, (long)(wave * EQ_TABLE_RECS | lane));
        if (own && !lt.eq.empty() && table[i][3] != 0u) fail("pad dword of an own record", x, y, k, (long)table[i][3], 0);
    }
    ++n_pairs;
    n_fast_columns += lt.eq.size();
    n_within += want >= 0;
    for (int p = 0; p < 2; ++p) for (int t = 0; t < 4; ++t) base_seen[p][t] += lt.base_seen[p][t];
    // blocks whose 96 positions [o, o + 96) pass the end of the pattern: the fast path starts at the first c0 with c0 - nv >= 0
    {
        int32_t a0 = lane_emin(d, k);
        if (a0 < -63) a0 = -63;
        const int nv = -a0;
        size_t blocks = lt.text.size() / 2, seen = 0;
        for (int c0 = 0; c0 + 32 <= n && seen < blocks; c0 += 32)
            if (c0 - nv >= 0) { ++seen; n_end_blocks += c0 - nv + 96 > m; }
    }
}

static std::string random_seq(int len)
{
    std::string s(len, 'A');
    for (int i = 0; i < len; ++i) s[i] = "ACGT"[rnd(4)];
    return s;
}

// y of length n out of x: random deletions or insertions down / up to n, then `subs` substitutions
static std::string derive(const std::string &x, int n, int subs)
{
    std::string y = x;
    while ((int)y.size() > n) y.erase(rnd((uint32_t)y.size()), 1);
    while ((int)y.size() < n) y.insert(rnd((uint32_t)y.size() + 1), 1, "ACGT"[rnd(4)]);
    for (int s = 0; s < subs && !y.empty(); ++s) {
        const uint32_t p = rnd((uint32_t)y.size());
        y[p] = "ACGT"[(std::strchr("ACGT", y[p]) - "ACGT" + 1 + rnd(3)) & 3];
    }
    return y;
}

int main(int argc, char **argv)
{
    const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;
    static const int LEN[] = {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257};
    static const int KS[] = {0, 1, 31, 32, 62, 63};
    // the length grid with every threshold that admits the pair; distances below, at and above the threshold
    for (int m : LEN) for (int n : LEN) for (int k : KS) {
        const int ad = m > n ? m - n : n - m;
        if (ad > k) continue;
        const std::string x = random_seq(m);
        const int room = k - ad;
        const int subs[] = {0, room / 2, room, room + 1, room + 3};
        for (int s : subs) {
            one_pair(x, derive(x, n, s), k);
            one_pair(derive(x, n, s), x, k);
        }
        one_pair(x, random_seq(n), k);
    }
    // one base throughout the text: every column of a block picks the same record, at even and at odd columns alike; and texts of period 2
    // and 4, which give each parity its own base
    for (int t = 0; t < 4; ++t) for (int m : {64, 97, 129, 257}) for (int k : {0, 1, 32, 63}) {
        const std::string x = random_seq(m);
        std::string y(m, "ACGT"[t]), y2(m, 'A'), y4(m, 'A');
        for (int i = 0; i < m; ++i) { y2[i] = "ACGT"[(t + (i & 1) * (1 + t % 3)) & 3]; y4[i] = "ACGT"[(t + i) & 3]; }
        one_pair(x, y, k); one_pair(y, y, k); one_pair(y, derive(y, m, 2), k);
        one_pair(x, y2, k); one_pair(y2, derive(y2, m, 1), k);
        one_pair(x, y4, k); one_pair(y4, derive(y4, m, 1), k);
    }
    // random pairs, a few of them long
    const int n_random = quick ? 300 : 4000;
    for (int i = 0; i < n_random; ++i) {
        const int m = 1 + (int)rnd(i % 50 == 0 ? 3000 : 700), k = (int)rnd(64);
        const int delta = (int)rnd(2 * (uint32_t)std::min(k, 8) + 1) - std::min(k, 8);
        const int n = std::max(1, m + delta);
        const std::string x = random_seq(m);
        const std::string y = rnd(8) == 0 ? random_seq(n) : derive(x, n, (int)rnd((uint32_t)k + 4));
        one_pair(x, y, k);
    }
    for (int p = 0; p < 2; ++p) for (int t = 0; t < 4; ++t)
        if (base_seen[p][t] < 1000) { std::printf("FAIL base %d at %s columns seen only %llu times\n", t, p ? "odd" : "even", (unsigned long long)base_seen[p][t]); return 1; }
    std::printf("ok %llu %llu %llu %llu\n", (unsigned long long)n_pairs, (unsigned long long)n_fast_columns, (unsigned long long)n_end_blocks,
                (unsigned long long)n_within);
    return 0;
}
