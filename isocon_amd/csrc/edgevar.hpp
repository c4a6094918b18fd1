// edgevar.hpp -- kernels of the edge variants of the statistical test (isocon_edge_variants: edgevar_host.inc; lane math in
// edgevar_core.hpp).  Reference call sites: modules/hypothesis_test_module.py:99-110, modules/functions.py:89-146, :218-236.
//
//   k_ev_records   one wavefront per edge, the ops on the lanes in steps of 64.  Both lists are summed up first (columns, bases of t and
//                  of c, columns of ops other than '=', the two reductions that find the masked ends: ev_list) -- that decides `bad`,
//                  the orientation and the number of variants.  The chosen list is walked again: wave prefix sums give every op its
//                  columns and bases in front, a second prefix sum over the ops' variant counts the place of its first record.  The
//                  variants of a step are then dealt to the lanes 64 at a time -- a lane finds the op of its variant by a binary search
//                  over the lanes' offsets (6 shuffles) and fetches that op by 5 more, so one 'D' op of 400 columns is 400 variants on
//                  64 lanes, not a loop on one.  A lane writes its own record (32 bytes; a wavefront's records are contiguous).  The
//                  per-op prefix sums of the chosen list are kept for the second launch.  An edge with more variants than its
//                  capacity gets its count and no record.
//   k_ev_snippets  one wavefront per edge, its variants on the lanes: both snippets of a variant byte by byte from the ops and the
//                  sequences (ev_snippet: the op of the first column by a binary search over the kept prefix sums); the gapped rows
//                  never exist.  Where a snippet starts comes from a prefix sum over the records' lengths made between the launches.
// No LDS, no scratch, no inline assembly.
#pragma once
#include "common.hpp"
#include "edgevar_core.hpp"

namespace isocon {

struct EvEdges {
    const uint8_t *seqs;              // the sequences' bytes
    const uint64_t *seq_ptr;          // n_seqs + 1
    const uint32_t *edge_t, *edge_c;  // ids into seqs
    const uint32_t *ops;
    const uint64_t *ops_ptr;          // 2 n + 1: list 2 e = (t, c), list 2 e + 1 = (c, t)
    const uint64_t *rec_ptr;          // n + 1: the record slots of edge e
    uint32_t n;
};

template <class T>
__device__ __forceinline__ T ev_wave_exscan(T v, uint32_t lane, T &total)
{
    T inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

__device__ __forceinline__ unsigned long long ev_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long ev_wave_min(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long ev_wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// one list summed up by a wavefront (every lane returns the same)
__device__ __forceinline__ EvList ev_wave_list(const uint32_t *__restrict__ ops, uint64_t n_ops, bool flipped, uint64_t len_t, uint64_t len_c, uint32_t lane)
{
    const uint32_t code_first = n_ops ? ev_code(ops[0]) : 0u, code_last = n_ops ? ev_code(ops[n_ops - 1]) : 0u;
    unsigned long long col = 0, t_bases = 0, c_bases = 0, gap_x = 0, start_min = ~0ull, end_max = 0;
    bool ops_ok = true;
    for (uint64_t base = 0; base < n_ops; base += 64) {
        const bool in = base + lane < n_ops;
        const uint32_t op = in ? ops[base + lane] : 0u;
        const uint32_t len = ev_len(op), code = ev_code(op);
        ops_ok &= !in || ev_op_ok(op);
        unsigned long long total;
        const unsigned long long at = col + ev_wave_exscan<unsigned long long>(len, lane, total);
        if (in) {
            const unsigned long long s = ev_start_offer(code, code_first, at), e = ev_end_offer(code, code_last, at + len);
            start_min = s < start_min ? s : start_min;
            end_max = e > end_max ? e : end_max;
            t_bases += ev_t_step(len, code, flipped);
            c_bases += ev_c_step(len, code, flipped);
            gap_x += code != EV_EQ ? len : 0u;
        }
        col += total;
    }
    return ev_list(n_ops, code_first, code_last, col, ev_wave_sum(t_bases), ev_wave_sum(c_bases), ev_wave_sum(gap_x), ev_wave_min(start_min), ev_wave_max(end_max),
                   __ballot(!ops_ok) == 0, len_t, len_c);
}

// recs: 8 int32 per record slot (ev_pack); pcol / pt / pc: one entry per op of `ops`, written for the chosen list of an edge
__global__ __launch_bounds__(256) void k_ev_records(EvEdges E, uint8_t *__restrict__ flipped_out, uint32_t *__restrict__ n_var_out, uint8_t *__restrict__ bad_out,
                                                     int32_t *__restrict__ recs, uint32_t *__restrict__ pcol, uint32_t *__restrict__ pt, uint32_t *__restrict__ pc)
{
    const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t t0 = E.seq_ptr[E.edge_t[e]], c0 = E.seq_ptr[E.edge_c[e]];
    const uint64_t len_t = E.seq_ptr[E.edge_t[e] + 1] - t0, len_c = E.seq_ptr[E.edge_c[e] + 1] - c0;
    const uint8_t *t = E.seqs + t0, *c = E.seqs + c0;
    const uint64_t o0 = E.ops_ptr[2 * (uint64_t)e], o1 = E.ops_ptr[2 * (uint64_t)e + 1], o2 = E.ops_ptr[2 * (uint64_t)e + 2];
    const EvList tc = ev_wave_list(E.ops + o0, o1 - o0, false, len_t, len_c, lane);
    const EvList ct = ev_wave_list(E.ops + o1, o2 - o1, true, len_t, len_c, lane);
    const bool ok = tc.ok && ct.ok;
    const bool flipped = ok && ct.n_var < tc.n_var;
    const EvList L = flipped ? ct : tc;
    const uint64_t cap = E.rec_ptr[e + 1] - E.rec_ptr[e];
    if (lane == 0) {
        bad_out[e] = ok ? 0 : 1;
        flipped_out[e] = flipped ? 1 : 0;
        n_var_out[e] = ok ? (uint32_t)L.n_var : 0u;
    }
    if (!ok || L.n_var > cap) return;
    const uint64_t g0 = flipped ? o1 : o0, n_ops = flipped ? o2 - o1 : o1 - o0;
    const uint32_t *__restrict__ ops = E.ops + g0;
    const uint32_t start = (uint32_t)L.start, end = (uint32_t)L.end, cols = (uint32_t)L.cols;
    uint32_t col = 0, t_before = 0, c_before = 0;
    uint64_t slot = E.rec_ptr[e];
    for (uint64_t base = 0; base < n_ops; base += 64) {
        const bool in = base + lane < n_ops;
        const uint32_t op = in ? ops[base + lane] : 0u;
        EvOp o;
        o.len = ev_len(op);
        o.code = ev_code(op);
        uint32_t cols_step, t_step, c_step, n_step;
        o.col = col + ev_wave_exscan<uint32_t>(o.len, lane, cols_step);
        o.t = t_before + ev_wave_exscan<uint32_t>(ev_t_step(o.len, o.code, flipped), lane, t_step);
        o.c = c_before + ev_wave_exscan<uint32_t>(ev_c_step(o.len, o.code, flipped), lane, c_step);
        if (in) {
            pcol[g0 + base + lane] = o.col;
            pt[g0 + base + lane] = o.t;
            pc[g0 + base + lane] = o.c;
        }
        const uint32_t mine = in && o.code != EV_EQ ? ev_overlap(o.col, o.len, start, end) : 0u;
        const uint32_t first = ev_wave_exscan<uint32_t>(mine, lane, n_step);          // this op's first variant among the step's
        for (uint32_t k = 0; k < n_step; k += 64) {
            const uint32_t j = k + lane;
            uint32_t a = 0, b = 64;          // the last lane whose first variant is <= j: it holds variant j (lanes without variants share their successor's offset)
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const uint32_t mid = (a + b) >> 1;
                if (__shfl(first, (int)mid, 64) <= j) a = mid; else b = mid;
            }
            EvOp w;
            w.len = __shfl(o.len, (int)a, 64);
            w.code = __shfl(o.code, (int)a, 64);
            w.col = __shfl(o.col, (int)a, 64);
            w.t = __shfl(o.t, (int)a, 64);
            w.c = __shfl(o.c, (int)a, 64);
            const uint32_t w_first = __shfl(first, (int)a, 64);
            if (j < n_step) {
                const uint32_t i = (w.col > start ? w.col : start) + (j - w_first);
                const EvRec r = ev_variant(t, (int32_t)len_t, c, (int32_t)len_c, flipped, w, i, cols);
                ev_pack(r, recs + (slot + j) * 8);
            }
        }
        slot += n_step;
        col += cols_step;
        t_before += t_step;
        c_before += c_step;
    }
}

// snip_ptr: one entry per record slot (+ 1); out_c / out_t: the bytes of aln_c / aln_t
__global__ __launch_bounds__(256) void k_ev_snippets(EvEdges E, const uint8_t *__restrict__ flipped_in, const uint32_t *__restrict__ n_var_in, const int32_t *__restrict__ recs,
                                                      const uint32_t *__restrict__ pcol, const uint32_t *__restrict__ pt, const uint32_t *__restrict__ pc,
                                                      const uint64_t *__restrict__ snip_ptr, uint8_t *__restrict__ out_c, uint8_t *__restrict__ out_t)
{
    const uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E.n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t slot0 = E.rec_ptr[e], cap = E.rec_ptr[e + 1] - slot0;
    const uint32_t n_var = n_var_in[e];
    if (n_var == 0 || n_var > cap) return;
    const bool flipped = flipped_in[e] != 0;
    const uint8_t *t = E.seqs + E.seq_ptr[E.edge_t[e]], *c = E.seqs + E.seq_ptr[E.edge_c[e]];
    const uint64_t g0 = E.ops_ptr[2 * (uint64_t)e + (flipped ? 1 : 0)], n_ops = E.ops_ptr[2 * (uint64_t)e + (flipped ? 2 : 1)] - g0;
    for (uint32_t v = lane; v < n_var; v += 64) {
        const int32_t *r = recs + (slot0 + v) * 8;
        const uint32_t i = (uint32_t)r[0], n = (uint32_t)r[6];
        const uint64_t at = snip_ptr[slot0 + v];
        ev_snippet(E.ops + g0, pcol + g0, pt + g0, pc + g0, (uint32_t)n_ops, flipped, t, c, i > 0 ? i - 1 : 0u, n, out_c + at, out_t + at);
    }
}

}  // namespace isocon
