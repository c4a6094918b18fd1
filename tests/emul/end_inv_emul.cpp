// Stand-alone driver of isocon_amd/csrc/end_inv_core.hpp (tests/test_end_inv_core.py; g++, also under -fsanitize=undefined,address).
//   end_inv_emul <thr>   then on stdin: n, and n sequences in ascending length order, one per line (at most four distinct symbols)
// The sequences are packed into bit planes as the store packs them -- planes[((chunk * n) + id) * 2 + plane], bases past the end 0,
// nchunks = ceil(maxlen / 64) + 1 -- in a heap array of EXACTLY nchunks * n * 2 words, so that a chunk index one past the end is an error
// of the sanitized build.  Then the core's rule runs over every window pair.
//   output: one line per entry "i p p ..." (the invariant partners of row i, ascending), then "# pairs survivors verified invariant"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../isocon_amd/csrc/end_inv_core.hpp"

using namespace isocon;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: end_inv_emul <thr> < sequences\n"); return 2; }
    const int32_t thr = (int32_t)strtol(argv[1], nullptr, 10);
    size_t n_in = 0;
    if (!(std::cin >> n_in)) return 2;
    std::vector<std::string> seqs(n_in);
    for (auto &s : seqs)
        if (!(std::cin >> s)) { fprintf(stderr, "expected %zu sequences\n", n_in); return 2; }
    const uint32_t n = (uint32_t)n_in;
    // the symbol map: "ACGT" where it fits, else the set's own symbols in byte order
    int code[256];
    for (int &c : code) c = -1;
    bool acgt = true;
    for (const auto &s : seqs) for (unsigned char ch : s) acgt = acgt && strchr("ACGT", ch) != nullptr;
    if (acgt) { code['A'] = 0; code['C'] = 1; code['G'] = 2; code['T'] = 3; }
    else {
        bool seen[256] = {false};
        for (const auto &s : seqs) for (unsigned char ch : s) seen[ch] = true;
        int next = 0;
        for (int ch = 0; ch < 256; ++ch) if (seen[ch]) code[ch] = next++;
        if (next > 4) { fprintf(stderr, "more than four distinct symbols\n"); return 3; }
    }
    std::vector<int32_t> lens(n);
    int32_t maxlen = 0;
    for (uint32_t i = 0; i < n; ++i) {
        lens[i] = (int32_t)seqs[i].size();
        if (i && lens[i] < lens[i - 1]) { fprintf(stderr, "not in ascending length order\n"); return 3; }
        if (lens[i] <= thr) { fprintf(stderr, "a sequence is not longer than thr\n"); return 3; }
        maxlen = lens[i] > maxlen ? lens[i] : maxlen;
    }
    const uint32_t nchunks = (uint32_t)((maxlen + 63) / 64) + 1u;
    const size_t words = (size_t)nchunks * n * 2;
    uint64_t *planes = new uint64_t[words]();          // (exactly sized, on the heap)
    for (uint32_t i = 0; i < n; ++i)
        for (int32_t t = 0; t < lens[i]; ++t) {
            const uint64_t c = (uint64_t)code[(unsigned char)seqs[i][t]];
            const size_t at = ((size_t)(t >> 6) * n + i) * 2;
            planes[at] |= (c & 1ull) << (t & 63);
            planes[at + 1] |= (c >> 1) << (t & 63);
        }
    uint64_t pairs = 0, survivors = 0, verified = 0, invariant = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t lo, hi;
        einv_window(lens.data(), n, i, thr, lo, hi);
        if (!(lo <= i && i < hi && hi <= n)) { fprintf(stderr, "entry %u: window [%u, %u)\n", i, lo, hi); return 4; }
        printf("%u", i);
        for (uint32_t r = 0; r + 1u < hi - lo; ++r) {
            const uint32_t p = einv_slot_partner(i, lo, r);
            if (p >= n || p == i) { fprintf(stderr, "entry %u slot %u: partner %u\n", i, r, p); return 4; }
            ++pairs;
            if (einv_pair_invariant(planes, n, nchunks, lens.data(), i, p, thr, &survivors, &verified)) { printf(" %u", p); ++invariant; }
        }
        printf("\n");
    }
    printf("# %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", pairs, survivors, verified, invariant);
    delete[] planes;
    return 0;
}
