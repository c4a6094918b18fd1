// edgevar_core.hpp -- lane-level math of the edge variants of the statistical test (edgevar.hpp), shared with the CPU emulator of
// tests/emul (g++, also under UBSan + ASan).
//
// An edge is a candidate c and its reference t with their two semi-global alignments as run-length ops (len << 4 | code, codes 0 '=',
// 1 'X', 2 'I' = consumes the query, 3 'D' = consumes the reference: SW_alignment_module._ops_to_alignment): list 0 aligns (t, c) -- t is
// the query --, list 1 aligns (c, t).  What the reference computes on the two gapped rows aln_t / aln_c of an alignment
// (modules/hypothesis_test_module.py:99-110, modules/functions.py:218-236 get_mask_start_and_end, :89-146 get_variant_coordinates)
// becomes, with every op knowing the columns and the bases of t and of c in front of it:
//     masked ends        start = the columns of the run of gap ops of one kind the list opens with, end = cols - the same at its tail
//     variants           the columns i in [start, end) of the ops other than '=', in column order; their number decides the orientation
//                        (list 1 replaces list 0 only with strictly fewer)
//     t_last / c_last    bases of t / c in aln[:i + 1], minus one: the op's bases in front plus i - its first column where the op consumes
//                        the sequence, the bases in front minus one where it does not
//     type, u_v          c's row is a gap: 'D', u_v = the run of t[t_last] in t around t_last; t's row is a gap: 'I', u_v = 1 + the run of
//                        c[c_last] in t on both sides of the gap (after t_last, and from t_last downwards); else 'S', u_v = 1
//     keys               'D' (t_last, c_last + 1), 'I' (t_last + 1, c_last), 'S' (t_last, c_last)
//     snippets           aln_c / aln_t[max(0, i - 1) : i + u_v + 1], cut at the row's end; a byte of a row is the sequence's base or '-'
// '=' against 'X' is TRUSTED: the trace kernels set the two from the bytes (sg.hpp), a list that says '=' over differing bases yields no
// variant there.  A variant outside the masked ends always has a base of t and of c at or before it (the op in front of a gap op that is
// not part of an end run consumes the gapped sequence), so t_last and c_last are >= 0 and the reference's wrap of t_seq[-1::-1] cannot
// occur.  A list is refused (the edge is `bad`) unless its ops consume exactly len(t) and len(c), use the four codes and have no empty op.
#pragma once
#include "band_core.hpp"

namespace isocon {

enum : uint32_t { EV_EQ = 0, EV_X = 1, EV_I = 2, EV_D = 3 };

ISO_HD uint32_t ev_len(uint32_t op) { return op >> 4; }
ISO_HD uint32_t ev_code(uint32_t op) { return op & 15u; }
// the bases of t / of c that an op consumes; flipped: the list aligns (c, t)
ISO_HD uint32_t ev_t_step(uint32_t len, uint32_t code, bool flipped) { return code < 2u || code == (flipped ? EV_D : EV_I) ? len : 0u; }
ISO_HD uint32_t ev_c_step(uint32_t len, uint32_t code, bool flipped) { return code < 2u || code == (flipped ? EV_I : EV_D) ? len : 0u; }
ISO_HD bool ev_op_ok(uint32_t op) { return ev_code(op) <= 3u && ev_len(op) != 0u; }

// What a lane offers to the two reductions that find the masked ends: the first column of an op that differs from the list's first op
// (minimum: where the opening run ends), the column behind an op that differs from the list's last op (maximum: where the closing run starts).
ISO_HD uint64_t ev_start_offer(uint32_t code, uint32_t code_first, uint64_t col) { return code != code_first ? col : ~0ull; }
ISO_HD uint64_t ev_end_offer(uint32_t code, uint32_t code_last, uint64_t col_end) { return code != code_last ? col_end : 0ull; }

// One list once its ops have been summed up.
struct EvList {
    uint64_t cols, start, end, n_var;
    bool ok;
};
// n_ops, the first and the last code, the sums over the ops (columns, bases of t, bases of c, columns of ops other than '='), the two
// reductions above and whether every op passed ev_op_ok
ISO_HD EvList ev_list(uint64_t n_ops, uint32_t code_first, uint32_t code_last, uint64_t cols, uint64_t t_bases, uint64_t c_bases, uint64_t gap_x_cols, uint64_t start_min,
                      uint64_t end_max, bool ops_ok, uint64_t len_t, uint64_t len_c)
{
    EvList L{cols, 0, cols, 0, false};
    L.ok = n_ops != 0 && ops_ok && t_bases == len_t && c_bases == len_c && len_t != 0 && len_c != 0;
    if (!L.ok) return L;
    if (code_first >= EV_I) L.start = start_min < cols ? start_min : cols;
    if (code_last >= EV_I) L.end = end_max;
    // (both sequences are consumed, so the list holds two kinds of ops or one that consumes both: start <= end, and the end runs are
    // gap ops -- columns of gap_x_cols)
    L.n_var = gap_x_cols - L.start - (cols - L.end);
    return L;
}

// columns of [col, col + len) inside [start, end)
ISO_HD uint32_t ev_overlap(uint32_t col, uint32_t len, uint32_t start, uint32_t end)
{
    const uint32_t a = col > start ? col : start, b = col + len < end ? col + len : end;
    return b > a ? b - a : 0u;
}

// An op of the chosen list with what lies in front of it.
struct EvOp {
    uint32_t len, code, col, t, c;          // columns, bases of t and bases of c before the op
};

struct EvRec {
    int32_t i, t_last, c_last, key_t, key_c, u_v, snip_len;
    uint8_t type, p_t, p_c;
};
// the record as the eight int32 of the C ABI: i, t_last, c_last, key on t, key on c, u_v, snippet length, type | p_t << 8 | p_c << 16
ISO_HD void ev_pack(const EvRec &r, int32_t *out)
{
    out[0] = r.i; out[1] = r.t_last; out[2] = r.c_last; out[3] = r.key_t; out[4] = r.key_c; out[5] = r.u_v; out[6] = r.snip_len;
    out[7] = (int32_t)((uint32_t)r.type | (uint32_t)r.p_t << 8 | (uint32_t)r.p_c << 16);
}

// length of the run of v in s[from ...] upwards / in s[... from] downwards
ISO_HD int32_t ev_run_up(const uint8_t *s, int32_t len, int32_t from, uint8_t v)
{
    int32_t k = from < 0 ? 0 : from;
    while (k < len && s[k] == v) ++k;
    return k - (from < 0 ? 0 : from);
}
ISO_HD int32_t ev_run_down(const uint8_t *s, int32_t len, int32_t from, uint8_t v)
{
    int32_t k = from < len ? from : len - 1;
    const int32_t top = k;
    while (k >= 0 && s[k] == v) --k;
    return top - k;
}

// The variant in column i of op o (a column of the op, the op not '='); cols: the length of the rows.
ISO_HD EvRec ev_variant(const uint8_t *t, int32_t len_t, const uint8_t *c, int32_t len_c, bool flipped, const EvOp &o, uint32_t i, uint32_t cols)
{
    const int32_t d = (int32_t)(i - o.col);
    const bool t_has = ev_t_step(1u, o.code, flipped) != 0u, c_has = ev_c_step(1u, o.code, flipped) != 0u;
    EvRec r;
    r.i = (int32_t)i;
    r.t_last = t_has ? (int32_t)o.t + d : (int32_t)o.t - 1;
    r.c_last = c_has ? (int32_t)o.c + d : (int32_t)o.c - 1;
    const bool t_in = r.t_last >= 0 && r.t_last < len_t, c_in = r.c_last >= 0 && r.c_last < len_c;          // (always, see above; never index outside)
    r.p_t = t_has && t_in ? t[r.t_last] : (uint8_t)'-';
    r.p_c = c_has && c_in ? c[r.c_last] : (uint8_t)'-';
    if (!c_has) {                    // the candidate lacks a base of t
        const uint8_t v = t_in ? t[r.t_last] : (uint8_t)0;
        r.type = 'D';
        r.u_v = ev_run_up(t, len_t, r.t_last + 1, v) + ev_run_down(t, len_t, r.t_last, v);          // (the run downwards holds t_last itself)
        if (r.u_v < 1) r.u_v = 1;
        r.key_t = r.t_last;
        r.key_c = r.c_last + 1;
    } else if (!t_has) {             // the candidate has an extra base
        const uint8_t v = c_in ? c[r.c_last] : (uint8_t)0;
        r.type = 'I';
        r.u_v = ev_run_up(t, len_t, r.t_last + 1, v) + (r.t_last >= 0 ? ev_run_down(t, len_t, r.t_last, v) : 0) + 1;
        r.key_t = r.t_last + 1;
        r.key_c = r.c_last;
    } else {
        r.type = 'S';
        r.u_v = 1;
        r.key_t = r.t_last;
        r.key_c = r.c_last;
    }
    const int64_t lo = i > 0 ? (int64_t)i - 1 : 0, hi = (int64_t)i + r.u_v + 1 < (int64_t)cols ? (int64_t)i + r.u_v + 1 : (int64_t)cols;
    r.snip_len = (int32_t)(hi - lo);
    return r;
}

// The columns [lo, lo + n) of both rows (lo + n <= the rows' length), each byte from the ops and the sequences: out_c / out_t[j] = column
// lo + j of aln_c / aln_t.  pcol / pt / pc: per op of the list the columns and the bases of t and of c before it.
ISO_HD void ev_snippet(const uint32_t *ops, const uint32_t *pcol, const uint32_t *pt, const uint32_t *pc, uint32_t n_ops, bool flipped, const uint8_t *t, const uint8_t *c,
                       uint32_t lo, uint32_t n, uint8_t *out_c, uint8_t *out_t)
{
    uint32_t a = 0, b = n_ops;          // the last op with pcol <= lo: pcol[a] <= lo, and pcol[b] > lo or b == n_ops
    while (b - a > 1u) {
        const uint32_t mid = a + (b - a) / 2u;
        if (pcol[mid] <= lo) a = mid; else b = mid;
    }
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t x = lo + j;
        while (a + 1u < n_ops && x >= pcol[a] + ev_len(ops[a])) ++a;
        const uint32_t code = ev_code(ops[a]), d = x - pcol[a];
        out_t[j] = ev_t_step(1u, code, flipped) ? t[pt[a] + d] : (uint8_t)'-';
        out_c[j] = ev_c_step(1u, code, flipped) ? c[pc[a] + d] : (uint8_t)'-';
    }
}

}  // namespace isocon
