// CPU emulation of one lane (one pair) of the banded global alignment path kernels (isocon_amd/csrc/nw_band.hpp) on the SAME lane-level
// math header (nw_band_core.hpp): the class and the window origin from the known distance, the forward pass through the sliding window
// with the [column][word] trace store, the score on the final diagonal, the masked walk with its reversed runs and the forward list made
// from them.  The text is the whole target or a window of it (start, columns), read unaligned as the kernel reads it.
// Test infrastructure for the not-gpu suite.
// With -DNWB_EMUL_MAIN the file is a stand-alone program (the sanitizer build): it reads cases "q t start cols ed last" from standard
// input (a '-' is the empty sequence) and prints "class ed op op ..." per case.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../isocon_amd/csrc/nw_band_core.hpp"

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
    int bit(int plane, long p) const
    {
        if (p < 0 || p >= len) return 0;
        return (int)(((plane ? hi : lo)[p >> 6] >> (p & 63)) & 1);
    }
    // 32 bits of a plane from position p on, zeros outside the sequence (hw_text32)
    uint32_t word32(int plane, long p) const
    {
        uint32_t w = 0;
        for (int b = 0; b < 32; ++b) w |= (uint32_t)bit(plane, p + b) << b;
        return w;
    }
    int base(long p) const { return bit(0, p) | (bit(1, p) << 1); }
};

struct Unit { uint64_t vp, hp; };

template <int W>
static int32_t run_band(const Planes &Q, const Planes &T, int32_t ts, int32_t n, int32_t ed, bool last, std::vector<uint32_t> &rev, int32_t *runs)
{
    const int32_t m = Q.len, a0 = nwb_origin(m - n, ed, W, last);
    std::vector<Unit> trace((size_t)n * W);
    const int32_t sc = nwb_forward<W>(
        [&](int plane, int32_t p) { return Q.word32(plane, p); }, [&](int plane, int32_t p) { return T.word32(plane, (long)ts + p); }, m, n, a0, true,
        [&](int32_t col, int w, uint64_t vp, uint64_t hp) { trace.at((size_t)col * W + w) = Unit{vp, hp}; }, [](bool b) { return b; });
    if (sc != ed) return sc < 0 ? -5 : sc;
    auto side = [&](int32_t j, int32_t w, uint64_t &vp, uint64_t &hp) { const Unit &u = trace.at((size_t)(j - 1) * W + w); vp = u.vp; hp = u.hp; };
    auto load = [&](int32_t, int32_t j, int32_t w, uint64_t &vp, uint64_t &hp) { side(j, w, vp, hp); };
    *runs = nwb_walk<W>(m, n, a0, load, side, [&](int32_t i, int32_t j) { return Q.base(i - 1) == T.base((long)ts + j - 1); },
                        [&](int32_t code, int32_t len) { rev.push_back(nwp_op(code, len)); });
    return sc;
}

// The pair (q, t[start .. start + cols)) of known distance ed.  ops: room for m + cols + 1.  *cls = the class W (0: not banded, nothing
// else is done).  Returns the pass' score (must equal ed), or the kernels' internal status: -5 the walk left the window, -6 more than
// 2 ed + 1 runs, -7 the window is not inside the target.  *n_ops forward ops, *n_rev reversed runs.  last: the window's other placement.
extern "C" int32_t emul_nw_band(const char *q, int m, const char *t, int nt, int start, int cols, int ed, int last, uint32_t *ops, int64_t *n_ops,
                                int64_t *n_rev, int32_t *cls)
{
    *n_ops = 0; *n_rev = 0; *cls = 0;
    if (start < 0 || cols < 0 || cols > nt - start) return -7;
    if (m <= 0 || cols <= 0) {          // the host's answer (nw_path_host.inc)
        if (m > 0) ops[(*n_ops)++] = nwp_op(NWP_I, m);
        if (cols > 0) ops[(*n_ops)++] = nwp_op(NWP_D, cols);
        return m > cols ? m : cols;
    }
    const int32_t W = nwb_class(m - cols, ed);
    *cls = W;
    if (!W) return ed;
    Planes Q, T;
    Q.set(q, m); T.set(t, nt);
    std::vector<uint32_t> rev;
    int32_t runs = 0;
    const int32_t sc = W == 1 ? run_band<1>(Q, T, start, cols, ed, last != 0, rev, &runs)
                     : W == 2 ? run_band<2>(Q, T, start, cols, ed, last != 0, rev, &runs) : run_band<4>(Q, T, start, cols, ed, last != 0, rev, &runs);
    if (sc != ed) return sc;
    if (runs < 0) return runs;
    if (runs != (int32_t)rev.size() || (uint64_t)runs > nwp_max_runs(ed)) return -6;
    *n_rev = runs;
    *n_ops = (int64_t)nwp_forward_runs(rev.data(), rev.size(), ops);
    return sc;
}

extern "C" int32_t emul_nwb_class(int32_t d, int32_t ed) { return nwb_class(d, ed); }

#ifdef NWB_EMUL_MAIN
int main()
{
    static char qb[1 << 16], tb[1 << 16];
    int start, cols, ed, last;
    while (scanf("%65535s %65535s %d %d %d %d", qb, tb, &start, &cols, &ed, &last) == 6) {
        const std::string q = strcmp(qb, "-") ? qb : "", t = strcmp(tb, "-") ? tb : "";
        std::vector<uint32_t> ops(q.size() + t.size() + 2);
        int64_t n_ops = 0, n_rev = 0;
        int32_t cls = 0;
        const int32_t sc = emul_nw_band(q.c_str(), (int)q.size(), t.c_str(), (int)t.size(), start, cols, ed, last, ops.data(), &n_ops, &n_rev, &cls);
        printf("%d %d", cls, sc);
        for (int64_t i = 0; i < n_ops; ++i) printf(" %u", ops[i]);
        printf("\n");
    }
    return 0;
}
#endif
