// Stand-alone driver of isocon_amd/csrc/msa_place_core.hpp (tests/test_msa_place_core.py; g++, also under -fsanitize=undefined,address).
//   msa_place_emul place   stdin: n, then n lines "representative insertion" (ACGT; 2 <= len(representative) <= 62, 1 <= len(insertion) <=
//                          len(representative)); output per line "columns outcome": the len + 2 columns of the placement and the step that
//                          gave them (0 substring, 1 threaded, 2 offset p > 0, 3 left-aligned)
//   msa_place_emul rep     stdin: n, then n lines "k s1 .. sk" (equally long insertions of one slot, in any order); output per line the
//                          representative as the two-key minimum leaves it
// A record is placed the way k_msa_place places it, on 64 emulated lanes in lockstep: the ballot of step 1, the anti-diagonals of step 2 with
// the two previous diagonals per lane and the neighbour's values read before anybody rotates, the maximum over the offsets of step 3.  The
// DP bytes live in a heap array of EXACTLY PLACE_DP_BYTES, so that a cell outside it is an error of the sanitized build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../isocon_amd/csrc/msa_place_core.hpp"

using namespace isocon;

static int code_of(char c)
{
    const char *at = strchr("ACGT", c);
    if (!at || !c) { fprintf(stderr, "not a base: %c\n", c); exit(3); }
    return (int)(at - "ACGT");
}

// the planes of a string (base j at bit j) as the kernels assemble them by ballot
static PlaceStr planes_of(const std::string &s)
{
    PlaceStr q = {0, 0, 0};
    for (size_t j = 0; j < s.size(); ++j) {
        const uint64_t c = (uint64_t)code_of(s[j]);
        q.v |= 1ull << j; q.b0 |= (c & 1ull) << j; q.b1 |= (c >> 1) << j;
    }
    return q;
}

// the wide record's code word of a string (base j at bits 2 j, the first 32 bases)
static uint64_t record_codes(const std::string &s)
{
    uint64_t codes = 0;
    for (size_t j = 0; j < s.size() && j < 32; ++j) codes |= (uint64_t)code_of(s[j]) << (2 * j);
    return codes;
}

static int place_wave(const PlaceStr &mx, int L, const PlaceStr &q, int m, uint8_t *D, PlaceStr &o)
{
    uint64_t found = 0;          // step 1: ballot
    for (int lane = 0; lane < 64; ++lane)
        if (lane <= L - m && place_eq(mx, q, lane) == q.v) found |= 1ull << lane;
    if (found) { o = place_at(q, __builtin_ctzll(found)); return PLACE_SUBSTRING; }
    uint32_t prev[64] = {0}, prev2[64] = {0}, cur[64] = {0};          // step 2
    for (int d = 2; d <= L + m; ++d) {
        uint32_t left_in[64], diag_in[64];
        for (int lane = 0; lane < 64; ++lane) { left_in[lane] = lane ? prev[lane - 1] : 0u; diag_in[lane] = lane ? prev2[lane - 1] : 0u; }          // (shuffles: before the branch)
        for (int lane = 0; lane < 64; ++lane) {
            const int j = lane + 1, i = d - j;
            if (j <= m && i >= 1 && i <= L) {
                const uint32_t up = i == 1 ? (uint32_t)j : prev[lane];
                const uint32_t left = lane == 0 ? (uint32_t)i : left_in[lane];
                const uint32_t diag = lane == 0 ? (uint32_t)(i - 1) : i == 1 ? (uint32_t)(j - 1) : diag_in[lane];
                cur[lane] = place_dp_value(up, left, diag, mx, q, i, j);
                D[place_dp_index(i, j)] = (uint8_t)cur[lane];
            }
        }
        for (int lane = 0; lane < 64; ++lane) { prev2[lane] = prev[lane]; prev[lane] = cur[lane]; }
    }
    if (place_thread(D, L, m, q, o)) return PLACE_THREADED;
    uint32_t best = 0;          // step 3: maximum over the lanes
    for (int lane = 0; lane < 64; ++lane) {
        const uint32_t key = lane <= L - m ? place_offset_key(mx, q, lane) : 0u;
        best = key > best ? key : best;
    }
    const int p = place_offset_of_key(best);
    o = place_at(q, p);
    return p > 0 ? PLACE_OFFSET : PLACE_LEFT;
}

// the slot's two keys after both passes over its records (atomicMin in any order: a minimum)
static std::string representative(const std::vector<std::string> &ins)
{
    const int n = (int)ins[0].size();
    uint64_t k1 = PLACE_KEY_NONE, k2 = PLACE_KEY_NONE;
    for (const auto &s : ins) { const uint64_t k = place_key_of_codes(record_codes(s)); k1 = k < k1 ? k : k1; }
    for (const auto &s : ins) {
        if (n <= 32 || place_key_of_codes(record_codes(s)) != k1) continue;
        const PlaceStr tail = planes_of(s.substr(32));
        const uint64_t k = place_key_of_planes(tail.b0, tail.b1, n - 32);
        k2 = k < k2 ? k : k2;
    }
    std::string out;
    for (int j = 0; j < n; ++j) out.push_back("ACGT"[place_key_code(k1, k2, j)]);
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 2 || (strcmp(argv[1], "place") && strcmp(argv[1], "rep"))) { fprintf(stderr, "usage: msa_place_emul place|rep < cases\n"); return 2; }
    size_t n = 0;
    if (!(std::cin >> n)) return 2;
    if (!strcmp(argv[1], "rep")) {
        for (size_t c = 0; c < n; ++c) {
            size_t k = 0;
            if (!(std::cin >> k) || k == 0) return 2;
            std::vector<std::string> ins(k);
            for (auto &s : ins) if (!(std::cin >> s) || s.size() != ins[0].size() || s.empty() || s.size() > (size_t)PLACE_MAX_LONGEST) return 3;
            printf("%s\n", representative(ins).c_str());
        }
        return 0;
    }
    uint8_t *D = new uint8_t[PLACE_DP_BYTES];          // (exactly sized, on the heap)
    std::string out;
    for (size_t c = 0; c < n; ++c) {
        std::string rep, ins;
        if (!(std::cin >> rep >> ins)) return 2;
        if (rep.size() < 2 || rep.size() > (size_t)PLACE_MAX_LONGEST || ins.empty() || ins.size() > rep.size()) { fprintf(stderr, "case %zu: lengths\n", c); return 3; }
        memset(D, 0xee, PLACE_DP_BYTES);
        const PlaceStr r = planes_of(rep), q = planes_of(ins);
        const int L = (int)rep.size() + 2;
        const PlaceStr mx = place_padded(r.b0, r.b1, (int)rep.size());
        PlaceStr o;
        const int outcome = place_wave(mx, L, q, (int)ins.size(), D, o);
        out.clear();
        for (int t = 0; t < L; ++t) out.push_back((char)place_char(o, t));
        printf("%s %d\n", out.c_str(), outcome);
    }
    delete[] D;
    return 0;
}
