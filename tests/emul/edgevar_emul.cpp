// CPU driver of isocon_amd/csrc/edgevar_core.hpp (tests/test_edgevar_core.py): k_ev_records and k_ev_snippets (edgevar.hpp) with 64
// emulated lanes -- the ops of a list on the lanes in steps of 64, wave prefix sums and reductions as loops over the lanes, the
// variants of a step dealt to the lanes by the same binary search over the lanes' offsets.  A program of its own (built with g++, and
// with -fsanitize=undefined,address): reads the edges from stdin, writes what the two kernels would to stdout.
//
//   in:   n_seqs, then one sequence per line; n_edges, then per edge: t c capacity n_ops0 ops0... n_ops1 ops1...
//   out:  per edge "E bad flipped n_var", then "OVER" (more variants than the capacity: no record) or per variant
//         "V i t_last c_last key_t key_c u_v type p_t p_c snippet_c snippet_t"
#include <stdint.h>
#include <stdio.h>
#include <iostream>
#include <string>
#include <vector>
#include "../../isocon_amd/csrc/edgevar_core.hpp"

using namespace isocon;

namespace {

constexpr int W = 64;

template <class T>
T exscan(const T *v, T *out)          // out[lane] = sum of v below the lane; returns the total
{
    T s = 0;
    for (int lane = 0; lane < W; ++lane) { out[lane] = s; s += v[lane]; }
    return s;
}

EvList wave_list(const uint32_t *ops, uint64_t n_ops, bool flipped, uint64_t len_t, uint64_t len_c)
{
    const uint32_t code_first = n_ops ? ev_code(ops[0]) : 0u, code_last = n_ops ? ev_code(ops[n_ops - 1]) : 0u;
    uint64_t col = 0, t_bases[W] = {}, c_bases[W] = {}, gap_x[W] = {}, start_min[W], end_max[W] = {};
    bool ops_ok[W];
    for (int lane = 0; lane < W; ++lane) { start_min[lane] = ~0ull; ops_ok[lane] = true; }
    for (uint64_t base = 0; base < n_ops; base += W) {
        uint64_t len[W], at[W];
        for (int lane = 0; lane < W; ++lane) len[lane] = base + lane < n_ops ? ev_len(ops[base + lane]) : 0u;
        const uint64_t total = exscan(len, at);
        for (int lane = 0; lane < W; ++lane) {
            if (!(base + lane < n_ops)) continue;
            const uint32_t op = ops[base + lane], code = ev_code(op);
            ops_ok[lane] = ops_ok[lane] && ev_op_ok(op);
            const uint64_t s = ev_start_offer(code, code_first, col + at[lane]), e = ev_end_offer(code, code_last, col + at[lane] + len[lane]);
            start_min[lane] = s < start_min[lane] ? s : start_min[lane];
            end_max[lane] = e > end_max[lane] ? e : end_max[lane];
            t_bases[lane] += ev_t_step((uint32_t)len[lane], code, flipped);
            c_bases[lane] += ev_c_step((uint32_t)len[lane], code, flipped);
            gap_x[lane] += code != EV_EQ ? len[lane] : 0u;
        }
        col += total;
    }
    uint64_t t_sum = 0, c_sum = 0, ne_sum = 0, mn = ~0ull, mx = 0;
    bool ok = true;
    for (int lane = 0; lane < W; ++lane) {
        t_sum += t_bases[lane]; c_sum += c_bases[lane]; ne_sum += gap_x[lane];
        mn = start_min[lane] < mn ? start_min[lane] : mn;
        mx = end_max[lane] > mx ? end_max[lane] : mx;
        ok = ok && ops_ok[lane];
    }
    return ev_list(n_ops, code_first, code_last, col, t_sum, c_sum, ne_sum, mn, mx, ok, len_t, len_c);
}

struct Edge {
    uint32_t t, c;
    uint64_t cap;
    std::vector<uint32_t> ops[2];
};

}  // namespace

int main()
{
    std::ios::sync_with_stdio(false);
    size_t n_seqs, n_edges;
    if (!(std::cin >> n_seqs)) return 2;
    std::vector<std::string> seqs(n_seqs);
    for (auto &s : seqs) std::cin >> s;
    if (!(std::cin >> n_edges)) return 2;
    std::string out;
    for (size_t e = 0; e < n_edges; ++e) {
        Edge E;
        std::cin >> E.t >> E.c >> E.cap;
        for (int l = 0; l < 2; ++l) {
            size_t n;
            std::cin >> n;
            E.ops[l].resize(n);
            for (auto &op : E.ops[l]) std::cin >> op;
        }
        if (!std::cin || E.t >= n_seqs || E.c >= n_seqs) return 2;
        const std::string &ts = seqs[E.t], &cs = seqs[E.c];
        const uint8_t *t = (const uint8_t *)ts.data(), *c = (const uint8_t *)cs.data();
        const uint64_t len_t = ts.size(), len_c = cs.size();
        // ---- k_ev_records ----
        const EvList tc = wave_list(E.ops[0].data(), E.ops[0].size(), false, len_t, len_c);
        const EvList ct = wave_list(E.ops[1].data(), E.ops[1].size(), true, len_t, len_c);
        const bool ok = tc.ok && ct.ok;
        const bool flipped = ok && ct.n_var < tc.n_var;
        const EvList L = flipped ? ct : tc;
        const uint64_t n_var = ok ? L.n_var : 0;
        out += "E " + std::to_string(ok ? 0 : 1) + " " + std::to_string(flipped ? 1 : 0) + " " + std::to_string(n_var) + "\n";
        if (!ok) continue;
        if (L.n_var > E.cap) { out += "OVER\n"; continue; }
        const std::vector<uint32_t> &ops = E.ops[flipped ? 1 : 0];
        const uint64_t n_ops = ops.size();
        std::vector<int32_t> recs((size_t)E.cap * 8);          // exactly the capacity: a record beyond it is a heap overflow (ASan)
        std::vector<uint32_t> pcol(n_ops), pt(n_ops), pc(n_ops);
        const uint32_t start = (uint32_t)L.start, end = (uint32_t)L.end, cols = (uint32_t)L.cols;
        uint32_t col = 0, t_before = 0, c_before = 0;
        uint64_t slot = 0;
        for (uint64_t base = 0; base < n_ops; base += W) {
            EvOp o[W];
            uint32_t len[W], ts_[W], cs_[W], a_col[W], a_t[W], a_c[W], mine[W], first[W];
            for (int lane = 0; lane < W; ++lane) {
                const uint32_t op = base + lane < n_ops ? ops[base + lane] : 0u;
                o[lane].len = len[lane] = ev_len(op);
                o[lane].code = ev_code(op);
                ts_[lane] = ev_t_step(len[lane], o[lane].code, flipped);
                cs_[lane] = ev_c_step(len[lane], o[lane].code, flipped);
            }
            const uint32_t cols_step = exscan(len, a_col), t_step = exscan(ts_, a_t), c_step = exscan(cs_, a_c);
            for (int lane = 0; lane < W; ++lane) {
                o[lane].col = col + a_col[lane];
                o[lane].t = t_before + a_t[lane];
                o[lane].c = c_before + a_c[lane];
                const bool in = base + lane < n_ops;
                if (in) { pcol[base + lane] = o[lane].col; pt[base + lane] = o[lane].t; pc[base + lane] = o[lane].c; }
                mine[lane] = in && o[lane].code != EV_EQ ? ev_overlap(o[lane].col, o[lane].len, start, end) : 0u;
            }
            const uint32_t n_step = exscan(mine, first);
            for (uint32_t k = 0; k < n_step; k += W)
                for (int lane = 0; lane < W; ++lane) {
                    const uint32_t j = k + lane;
                    uint32_t a = 0, b = W;
                    for (int it = 0; it < 6; ++it) {
                        const uint32_t mid = (a + b) >> 1;
                        if (first[mid] <= j) a = mid; else b = mid;
                    }
                    const EvOp w = o[a];
                    if (j < n_step) {
                        const uint32_t i = (w.col > start ? w.col : start) + (j - first[a]);
                        const EvRec r = ev_variant(t, (int32_t)len_t, c, (int32_t)len_c, flipped, w, i, cols);
                        ev_pack(r, recs.data() + (slot + j) * 8);
                    }
                }
            slot += n_step;
            col += cols_step;
            t_before += t_step;
            c_before += c_step;
        }
        if (slot != n_var) return 3;          // the emitted records are the counted ones
        // ---- k_ev_snippets ----
        for (uint64_t v = 0; v < n_var; ++v) {
            const int32_t *r = recs.data() + v * 8;
            const uint32_t i = (uint32_t)r[0], n = (uint32_t)r[6];
            std::vector<uint8_t> sc(n), st(n);          // exactly the record's length
            ev_snippet(ops.data(), pcol.data(), pt.data(), pc.data(), (uint32_t)n_ops, flipped, t, c, i > 0 ? i - 1 : 0u, n, sc.data(), st.data());
            char head[160];
            snprintf(head, sizeof head, "V %d %d %d %d %d %d %c %c %c ", r[0], r[1], r[2], r[3], r[4], r[5], (char)(r[7] & 255), (char)(r[7] >> 8 & 255), (char)(r[7] >> 16 & 255));
            out += head + std::string(sc.begin(), sc.end()) + " " + std::string(st.begin(), st.end()) + "\n";
        }
    }
    fputs(out.c_str(), stdout);
    return 0;
}
