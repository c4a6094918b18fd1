// CPU emulation of one wavefront (one pair) of the global alignment path kernels (isocon_amd/csrc/nw_path.hpp): 64 lanes in lock
// step on the SAME lane-level math headers (hw_full_core.hpp, nw_path_core.hpp) -- the TRACE pass over the whole target with every
// column kept in the [step][lane] store, passes of 64 blocks with the 2-bit boundary buffer, the walk of the whole path with its
// reversed runs, and the forward list made from them.  Test infrastructure for the not-gpu suite.
// With -DNWP_EMUL_MAIN the file is a stand-alone program (the sanitizer build): it reads cases "q t" from standard input (a '-' is the
// empty sequence) and prints "ed op op ..." per case.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../isocon_amd/csrc/nw_path_core.hpp"

using namespace isocon;

static inline int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

struct Planes {
    std::vector<uint64_t> lo, hi;
    int len = 0;
    void set(const char *s, int n)
    {
        len = n;
        const int nc = (n + 63) / 64 + 1;
        lo.assign(nc, 0); hi.assign(nc, 0);
        for (int i = 0; i < n; ++i) {
            const int c = code_of(s[i]);
            if (c & 1) lo[i >> 6] |= (uint64_t)1 << (i & 63);
            if (c & 2) hi[i >> 6] |= (uint64_t)1 << (i & 63);
        }
    }
    int base(long p) const { return (p < 0 || p >= len) ? 0 : (int)((lo[p >> 6] >> (p & 63)) & 1) | (int)(((hi[p >> 6] >> (p & 63)) & 1) << 1); }
};

struct Unit { uint64_t pv, ph; };

// The TRACE pass of the query against the whole target (the loop of hwf_run<HWF_TRACE> with keep_cols).  Returns the last row's score.
static int32_t trace_pass(const Planes &Q, const Planes &T, std::vector<Unit> &trace)
{
    const int32_t m = Q.len, ncols = T.len;
    const int32_t passes = hwf_passes(m);
    std::vector<uint32_t> bound(hwf_bound_words(ncols) + 1, 0);
    int32_t score = HWB_INF;
    for (int32_t pass = 0; pass < passes; ++pass) {
        const int32_t nbl = hwf_pass_lanes(m, pass);
        HwfLane L[64];
        int32_t packed[64], next[64];
        for (int l = 0; l < 64; ++l) {
            const int32_t blk = pass * 64 + l;
            const bool has = blk < (int32_t)Q.lo.size();
            hwf_lane_init(L[l], has ? Q.lo[blk] : 0, has ? Q.hi[blk] : 0, m, blk * 64);
            packed[l] = hwf_pack(0, 0);
        }
        uint32_t bw = 0;
        const int32_t steps = ncols + nbl - 1;
        for (int32_t s = 0; s < steps; ++s) {
            for (int l = 0; l < 64; ++l) {
                int32_t ch, hin;
                if (l == 0) {
                    ch = s < ncols ? T.base(s) : 0;
                    hin = pass == 0 ? 1 : (s < ncols ? hwf_bound_get(bound[s >> 4], s) : 0);
                } else {
                    ch = hwf_packed_base(packed[l - 1]);
                    hin = hwf_packed_delta(packed[l - 1]);
                }
                const int32_t col = s - l;
                int32_t hout = 0;
                if (col >= 0 && col < ncols && l < nbl) {
                    uint64_t ph;
                    hout = hwf_step<HWF_TRACE>(L[l], ch, hin, col, 0, ph);
                    trace[hwf_trace_unit(m, ncols, pass * 64 + l, col + 1)] = Unit{L[l].Pv, ph};
                    if (l == 63 && pass + 1 < passes) {
                        bw = hwf_bound_add(bw, col, hout);
                        if (hwf_bound_full(col, ncols)) { bound[col >> 4] = bw; bw = 0; }
                    }
                }
                next[l] = hwf_pack(ch, hout);
            }
            memcpy(packed, next, sizeof packed);
        }
        if (pass == passes - 1) score = L[((m - 1) >> 6) - pass * 64].score;
    }
    return score;
}

// ops: room for m + n + 1.  Returns the distance, *n_ops = number of forward ops; *n_rev = number of reversed runs the walk emitted.
extern "C" int32_t emul_nw_path(const char *q, int m, const char *t, int n, uint32_t *ops, int64_t *n_ops, int64_t *n_rev)
{
    *n_ops = 0; *n_rev = 0;
    if (m <= 0 || n <= 0) {          // the host's answer (nw_path_host.inc)
        if (m > 0) ops[(*n_ops)++] = nwp_op(NWP_I, m);
        if (n > 0) ops[(*n_ops)++] = nwp_op(NWP_D, n);
        return m > n ? m : n;
    }
    Planes Q, T;
    Q.set(q, m); T.set(t, n);
    std::vector<Unit> trace(hwf_trace_units(m, n));
    const int32_t ed = trace_pass(Q, T, trace);
    std::vector<uint32_t> rev;
    // the kernel's walk: a request names a block and 64 columns, the block's plane words and the columns' bases come with it
    int32_t b0 = -1, j0 = 0;
    const int32_t runs = nwp_walk(m, n,
        [&](int32_t b, int32_t j, uint64_t &pv, uint64_t &ph) {
            if (b != b0 || j > j0 || j <= j0 - 64) { b0 = b; j0 = j; }
            const Unit &u = trace[hwf_trace_unit(m, n, b, j)]; pv = u.pv; ph = u.ph;
        },
        [&](int32_t i, int32_t j) {
            const int32_t bit = (i - 1) & 63;
            if (((i - 1) >> 6) != b0 || j > j0 || j <= j0 - 64) return false;          // (outside the last request: a wrong answer, on purpose)
            const int qb = (int)((Q.lo[b0] >> bit) & 1) | (int)(((Q.hi[b0] >> bit) & 1) << 1);
            return qb == T.base(j - 1);
        },
        [&](int32_t code, int32_t len) { rev.push_back(nwp_op(code, len)); });
    if (runs != (int32_t)rev.size()) return -7;
    if ((uint64_t)runs > nwp_max_runs(ed)) return -6;
    *n_rev = runs;
    *n_ops = (int64_t)nwp_forward_runs(rev.data(), rev.size(), ops);
    return ed;
}

extern "C" int64_t emul_forward_runs(const uint32_t *rev, int64_t n_rev, uint32_t *fwd) { return (int64_t)nwp_forward_runs(rev, (uint64_t)n_rev, fwd); }

#ifdef NWP_EMUL_MAIN
int main()
{
    static char qb[1 << 16], tb[1 << 16];
    while (scanf("%65535s %65535s", qb, tb) == 2) {
        const std::string q = strcmp(qb, "-") ? qb : "", t = strcmp(tb, "-") ? tb : "";
        std::vector<uint32_t> ops(q.size() + t.size() + 2);
        int64_t n_ops = 0, n_rev = 0;
        const int32_t ed = emul_nw_path(q.c_str(), (int)q.size(), t.c_str(), (int)t.size(), ops.data(), &n_ops, &n_rev);
        printf("%d", ed);
        for (int64_t i = 0; i < n_ops; ++i) printf(" %u", ops[i]);
        printf("\n");
    }
    // the reversed-runs helper on its own: a single op, equal neighbours, an empty run between them
    const uint32_t one[1] = {nwp_op(NWP_EQ, 7)}, many[5] = {nwp_op(NWP_I, 2), nwp_op(NWP_I, 3), nwp_op(NWP_EQ, 0), nwp_op(NWP_I, 1), nwp_op(NWP_X, 4)};
    uint32_t out[5];
    if (nwp_forward_runs(one, 1, out) != 1 || out[0] != one[0]) return 3;
    if (nwp_forward_runs(many, 5, out) != 2 || out[0] != nwp_op(NWP_X, 4) || out[1] != nwp_op(NWP_I, 6) || nwp_forward_runs(many, 5, nullptr) != 2) return 4;
    return 0;
}
#endif
