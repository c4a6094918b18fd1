// Stand-alone driver of the pair-list plan (isocon_amd/csrc/ed_pairs_plan.hpp) and of the gathered upload's byte-range copy
// (gather_bytes in the same header) on the CPU.  Behind the plan's backend stand the emulators of band_emul.cpp (one tile, one lane: the
// kernels' own lane-level headers) and a textbook DP for the un-banded stage; every pair's answer is checked against the DP.
// Built together with band_emul.cpp by tests/test_ed_pairs_plan.py, plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../isocon_amd/csrc/ed_pairs_plan.hpp"

extern "C" void emul_band_tile(int W, const char *pat, int m, int nl, const char **texts, const int *tlens, const int *ks, int32_t *out);
extern "C" int32_t emul_ed_lane(const char *x, int m, const char *y, int n, int k);

static std::mt19937 rng(20240611u);
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

static int fail(const char *what, long long x = 0, long long y = 0, long long z = 0)
{
    printf("FAIL %s %lld %lld %lld\n", what, x, y, z);
    return 1;
}

static int32_t dp_distance(const std::string &x, const std::string &y)
{
    std::vector<int32_t> row(y.size() + 1);
    for (size_t j = 0; j <= y.size(); ++j) row[j] = (int32_t)j;
    for (size_t i = 1; i <= x.size(); ++i) {
        int32_t diag = row[0];
        row[0] = (int32_t)i;
        for (size_t j = 1; j <= y.size(); ++j) {
            const int32_t up = row[j];
            row[j] = std::min(std::min(up, row[j - 1]) + 1, diag + (x[i - 1] != y[j - 1]));
            diag = up;
        }
    }
    return row[y.size()];
}

struct Set {
    std::vector<std::string> seqs;
    std::map<std::pair<uint32_t, uint32_t>, int32_t> known;
    uint32_t add(const std::string &s) { seqs.push_back(s); return (uint32_t)seqs.size() - 1; }
    int32_t distance(uint32_t a, uint32_t b)
    {
        const auto key = std::make_pair(std::min(a, b), std::max(a, b));
        auto it = known.find(key);
        if (it == known.end()) it = known.emplace(key, dp_distance(seqs[a], seqs[b])).first;
        return it->second;
    }
};

// the stages on the CPU, with the number of pairs every call received
struct CpuStages {
    Set &set;
    uint64_t n_lanes = 0, n_round[2] = {0, 0}, n_w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, n_full = 0, minus2 = 0, n_w1_round0 = 0;
    int last_w = 0;
    bool bad_input = false;
    explicit CpuStages(Set &s) : set(s) {}
    int lanes(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, const std::vector<int32_t> &k, std::vector<int32_t> &out)
    {
        out.assign(a.size(), -1);
        n_lanes += a.size();
        for (size_t i = 0; i < a.size(); ++i) {
            const std::string &x = set.seqs[a[i]], &y = set.seqs[b[i]];
            if (k[i] < 0 || k[i] > 63) bad_input = true;
            out[i] = emul_ed_lane(x.data(), (int)x.size(), y.data(), (int)y.size(), k[i]);
        }
        return ISOCON_OK;
    }
    int tiles(int W, const std::vector<uint32_t> &ts, const std::vector<uint32_t> &ids, const std::vector<int32_t> &ks, std::vector<int32_t> &out)
    {
        const int round = W == last_w ? 1 : 0;          // the plan calls a stage's one-lane round right after its first
        last_w = W;
        if (ids.size() != ts.size() * 64 || ks.size() != ids.size() || (W != 1 && W != 2 && W != 4 && W != 8)) { bad_input = true; return ISOCON_E_ARG; }
        out.assign(ids.size(), -1);
        for (size_t t = 0; t < ts.size(); ++t) {
            std::vector<const char *> texts;
            std::vector<int> tlens, tk;
            std::vector<size_t> slot;
            for (size_t l = 0; l < 64; ++l) {
                const size_t s = t * 64 + l;
                if (ids[s] == 0xffffffffu) { if (ks[s] != -1) bad_input = true; continue; }
                if (ks[s] < 0 || ks[s] > 64 * W - 1 || (round == 1 && l > 0)) bad_input = true;
                n_round[round] += 1; n_w[W] += 1; n_w1_round0 += W == 1 && round == 0;
                // an empty sequence on either side: the kernel answers such a lane before its band starts (ed_band.hpp band_tile_run, `trivial`)
                const int m = (int)set.seqs[ts[t]].size(), n = (int)set.seqs[ids[s]].size(), ad = m > n ? m - n : n - m;
                if (m == 0 || n == 0) { out[s] = ad <= ks[s] ? ad : -1; continue; }
                texts.push_back(set.seqs[ids[s]].data());
                tlens.push_back((int)set.seqs[ids[s]].size());
                tk.push_back(ks[s]);
                slot.push_back(s);
            }
            if (ids[t * 64] == 0xffffffffu) bad_input = true;          // no tile without a lane, lanes fill a tile from its front
            if (slot.empty()) continue;
            std::vector<int32_t> res(slot.size(), -1);
            const std::string &pat = set.seqs[ts[t]];
            emul_band_tile(W, pat.data(), (int)pat.size(), (int)slot.size(), texts.data(), tlens.data(), tk.data(), res.data());
            for (size_t i = 0; i < slot.size(); ++i) { out[slot[i]] = res[i]; minus2 += res[i] == -2; }
        }
        return ISOCON_OK;
    }
    int full(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, const std::vector<int32_t> &k, std::vector<int32_t> &out)
    {
        out.assign(a.size(), -1);
        n_full += a.size();
        for (size_t i = 0; i < a.size(); ++i) {
            const int32_t d = set.distance(a[i], b[i]);
            out[i] = k[i] < 0 || d <= k[i] ? d : -1;
        }
        return ISOCON_OK;
    }
};

struct PairList {
    std::vector<uint32_t> a, b;
    std::vector<int32_t> k;
    void add(uint32_t x, uint32_t y, int32_t kk) { a.push_back(x); b.push_back(y); k.push_back(kk); }
};

static std::string random_seq(size_t len, const char *letters, uint32_t n_letters)
{
    std::string s(len, 'A');
    for (char &c : s) c = letters[rnd(n_letters)];
    return s;
}

// a copy of x with `edits` random substitutions, insertions and deletions
static std::string mutate(const std::string &x, int edits)
{
    std::string y = x;
    for (int e = 0; e < edits; ++e) {
        const uint32_t kind = rnd(3), pos = y.empty() ? 0 : rnd((uint32_t)y.size());
        if (kind == 0 && !y.empty()) y[pos] = "ACGT"[rnd(4)];
        else if (kind == 1 || y.empty()) y.insert(y.begin() + pos, "ACGT"[rnd(4)]);
        else y.erase(y.begin() + pos);
    }
    return y;
}

// x over {A, C}; y = x with `subs` positions turned into G and `dels` others removed: every G costs an edit of its own and the
// length difference `dels` more, so the distance is subs + dels exactly
static std::string plant(const std::string &x, int subs, int dels)
{
    std::vector<uint32_t> pos(x.size());
    for (size_t i = 0; i < pos.size(); ++i) pos[i] = (uint32_t)i;
    for (size_t i = 0; i + 1 < pos.size(); ++i) std::swap(pos[i], pos[i + rnd((uint32_t)(pos.size() - i))]);
    std::string y = x;
    for (int i = 0; i < subs; ++i) y[pos[i]] = 'G';
    for (int i = 0; i < dels; ++i) y[pos[subs + i]] = '-';
    y.erase(std::remove(y.begin(), y.end(), '-'), y.end());
    return y;
}

// runs the plan over the list and checks every answer; the counts of `st` are the caller's to print
static int run_list(Set &set, const PairList &pl, size_t min_group, CpuStages &st, uint64_t *within, uint64_t *beyond, uint64_t *full_pairs)
{
    std::vector<int32_t> lens;
    for (const std::string &s : set.seqs) lens.push_back((int32_t)s.size());
    const uint64_t np = pl.a.size();
    std::vector<uint64_t> pending(np);
    for (uint64_t p = 0; p < np; ++p) pending[p] = p;
    const int32_t unsettled = -7;
    std::vector<int32_t> out(np, unsettled);
    std::string error;
    const int rc = ed_pairs_plan(lens.data(), (uint32_t)lens.size(), pl.a.data(), pl.b.data(), pl.k.data(), np, pending, min_group, st, out.data(), full_pairs, error);
    if (rc) { printf("FAIL plan status %d (%s)\n", rc, error.c_str()); return 1; }
    if (st.bad_input) return fail("a stage received input outside its contract");
    if (*full_pairs != st.n_full) return fail("full_pairs", (long long)*full_pairs, (long long)st.n_full);
    for (uint64_t p = 0; p < np; ++p) {
        const int32_t d = set.distance(pl.a[p], pl.b[p]), want = pl.k[p] < 0 || d <= pl.k[p] ? d : -1;
        if (out[p] == unsettled) return fail("pair not settled", (long long)p);
        if (out[p] != want) return fail("pair, got, expected", (long long)p, out[p], want);
        ++*(want >= 0 ? within : beyond);
    }
    return 0;
}

static int check_plan()
{
    Set set;
    PairList pl;
    // one shared sequence with 1 .. 129 partners, thresholds around the partners' distances
    const int group_sizes[7] = {1, 15, 16, 17, 64, 65, 129};
    for (int g : group_sizes) {
        const uint32_t shared = set.add(random_seq(150 + rnd(100), "ACGT", 4));
        for (int i = 0; i < g; ++i) {
            const int edits = (int)rnd(40);
            const uint32_t partner = set.add(mutate(set.seqs[shared], edits));
            const int32_t d = set.distance(shared, partner);
            const int32_t ks[5] = {-1, d, d - 1, d + 1, 63};
            pl.add(shared, partner, ks[rnd(5)]);
        }
    }
    // 64 partners whose lengths differ from the shared sequence's by -63 .. +63, k = the distance: a tile cannot certify them all
    {
        const std::string x = random_seq(300, "AC", 2);
        const uint32_t shared = set.add(x);
        for (int delta = -63; delta <= 63; delta += 2) {
            const std::string y = delta < 0 ? plant(x, 0, -delta) : x;
            const uint32_t partner = set.add(delta > 0 ? y + std::string((size_t)delta, 'G') : y);
            pl.add(shared, partner, delta < 0 ? -delta : delta);
        }
    }
    // distances on both sides of every stage's cap, thresholds on both sides of the distances, both argument orders
    const int caps[4] = {63, 127, 255, 511};
    for (int cap : caps) {
        const std::string x = random_seq(cap == 511 ? 700 : 2 * cap + 100, "AC", 2);
        const uint32_t ix = set.add(x);
        for (int d = cap; d <= cap + 1; ++d) {
            const int dels = d % 7;
            const uint32_t iy = set.add(plant(x, d - dels, dels));
            if (set.distance(ix, iy) != d) return fail("planted distance", d, set.distance(ix, iy));
            const int32_t ks[4] = {d - 1, d, d + 1, -1};
            for (int32_t kk : ks) { pl.add(ix, iy, kk); pl.add(iy, ix, kk); }
        }
    }
    // empty sequences, on either side and on both
    {
        const uint32_t e0 = set.add(""), e1 = set.add(""), s = set.add(random_seq(40, "ACGT", 4)), l = set.add(random_seq(90, "ACGT", 4));
        pl.add(e0, e1, -1); pl.add(e0, e1, 0); pl.add(e0, e0, 5);
        pl.add(e0, s, -1); pl.add(s, e0, 40); pl.add(s, e1, 39); pl.add(e1, l, 63); pl.add(l, e0, -1); pl.add(e0, l, 100);
    }
    // the same pair twice in one list (one of them with another threshold as well)
    pl.add(pl.a[20], pl.b[20], pl.k[20]);
    pl.add(pl.a[300], pl.b[300], pl.k[300]);
    pl.add(pl.a[300], pl.b[300], -1);

    uint64_t within = 0, beyond = 0, full_pairs = 0, other_full = 0;
    CpuStages dflt(set), none(set), all(set), swapped(set);
    if (run_list(set, pl, 16, dflt, &within, &beyond, &full_pairs)) return 1;
    uint64_t w2 = 0, b2 = 0;
    if (run_list(set, pl, 0, none, &w2, &b2, &other_full)) return 1;
    if (none.n_lanes != 0) return fail("min_group 0 sent pairs to the lanes", (long long)none.n_lanes);
    if (run_list(set, pl, (size_t)-1, all, &w2, &b2, &other_full)) return 1;
    if (all.n_w[1] != 0 || all.n_lanes != pl.a.size()) return fail("unlimited min_group sent pairs to the 64-row tiles", (long long)all.n_w[1], (long long)all.n_lanes);
    // a list whose second side is the shared one: the groups again with the sides exchanged (tiled by its first side, every group would hold one pair
    // and go to the lanes)
    PairList sw;
    for (size_t p = 0; p < 307 + 64; ++p) sw.add(pl.b[p], pl.a[p], pl.k[p]);
    if (run_list(set, sw, 16, swapped, &w2, &b2, &other_full)) return 1;
    if (swapped.n_lanes != 1 + 15 || swapped.n_round[0] < 16 + 17 + 64 + 65 + 129 + 64) return fail("exchanged list: lanes, tiles", (long long)swapped.n_lanes, (long long)swapped.n_round[0]);

    printf("pairs %zu\nwithin %llu\nbeyond %llu\n", pl.a.size(), (unsigned long long)within, (unsigned long long)beyond);
    printf("lanes %llu\ntiles_round0 %llu\ntiles_round1 %llu\n", (unsigned long long)dflt.n_lanes, (unsigned long long)dflt.n_round[0], (unsigned long long)dflt.n_round[1]);
    printf("tiles_w1 %llu\ntiles_w2 %llu\ntiles_w4 %llu\ntiles_w8 %llu\n", (unsigned long long)dflt.n_w[1], (unsigned long long)dflt.n_w[2], (unsigned long long)dflt.n_w[4],
           (unsigned long long)dflt.n_w[8]);
    printf("full %llu\nminus2 %llu\n", (unsigned long long)dflt.n_full, (unsigned long long)dflt.minus2);
    printf("min_group0_tiles_w1 %llu\nunlimited_lanes %llu\nswapped_tiles_round0 %llu\n", (unsigned long long)none.n_w1_round0, (unsigned long long)all.n_lanes,
           (unsigned long long)swapped.n_round[0]);
    return 0;
}

// bytes [b0, b1) of the concatenation into a buffer of exactly b1 - b0 bytes (the sanitized build sees a byte written outside it)
static int check_range(const std::vector<const uint8_t *> &ptrs, const std::vector<uint64_t> &offsets, const std::string &cat, uint64_t b0, uint64_t b1)
{
    const size_t len = (size_t)(b1 - b0);
    std::unique_ptr<char[]> dst(new char[len]);
    for (size_t i = 0; i < len; ++i) dst[i] = '#';
    gather_bytes(dst.get(), ptrs.data(), offsets.data(), (uint32_t)ptrs.size(), b0, b1);
    if (len && memcmp(dst.get(), cat.data() + b0, len) != 0) return fail("gathered range", (long long)b0, (long long)b1);
    return 0;
}

static int check_gather()
{
    uint64_t ranges = 0, cuts = 0;
    for (uint64_t base : {(uint64_t)0, (uint64_t)1000}) {
        // runs of empty sequences at the front, in the middle and at the end
        const int lens[] = {0, 0, 5, 1, 0, 0, 0, 17, 64, 0, 3, 200, 0, 0};
        std::vector<std::string> seqs;
        std::vector<const uint8_t *> ptrs;
        std::vector<uint64_t> offsets(1, base);
        std::string cat;
        for (int l : lens) seqs.push_back(random_seq((size_t)l, "ACGTN", 5));
        for (const std::string &s : seqs) {
            ptrs.push_back(s.empty() ? nullptr : (const uint8_t *)s.data());
            offsets.push_back(offsets.back() + s.size());
            cat += s;
        }
        const uint64_t total = cat.size();
        // every range that starts and ends on a boundary or one byte off it
        std::vector<uint64_t> marks;
        for (uint64_t o : offsets)
            for (int delta = -1; delta <= 1; ++delta)
                if (o - base + delta <= total) marks.push_back(o - base + delta);          // (below zero wraps past total)
        for (uint64_t b0 : marks)
            for (uint64_t b1 : marks)
                if (b0 <= b1) { if (check_range(ptrs, offsets, cat, b0, b1)) return 1; ++ranges; }
        for (int i = 0; i < 300; ++i) {
            const uint64_t b0 = rnd((uint32_t)total + 1), b1 = b0 + rnd((uint32_t)(total - b0) + 1);
            if (check_range(ptrs, offsets, cat, b0, b1)) return 1;
            ++ranges;
        }
        // the whole range in 1 .. 4 parts cut at arbitrary bytes
        for (int parts = 1; parts <= 4; ++parts)
            for (int rep = 0; rep < 50; ++rep) {
                std::vector<uint64_t> cut = {0, total};
                for (int c = 1; c < parts; ++c) cut.push_back(rnd((uint32_t)total + 1));
                std::sort(cut.begin(), cut.end());
                for (size_t c = 0; c + 1 < cut.size(); ++c)
                    if (check_range(ptrs, offsets, cat, cut[c], cut[c + 1])) return 1;
                ++cuts;
            }
    }
    printf("gather_ranges %llu\ngather_cuts %llu\n", (unsigned long long)ranges, (unsigned long long)cuts);
    return 0;
}

int main()
{
    if (check_plan() || check_gather()) return 1;
    printf("ok 1\n");
    return 0;
}
