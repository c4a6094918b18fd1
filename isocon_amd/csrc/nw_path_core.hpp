// nw_path_core.hpp -- lane-level math of the GLOBAL ("NW") alignment path kernels (nw_path.hpp, gfx950): device side of
// edlib.align(q, t, mode="NW", task="path", k) for pair lists.  Specification: orc_nw_path (oracle/isocon_oracle.c section 5).
//
// The global alignment of the query (m rows) against the whole target (n columns) IS the TRACE pass of hw_full_core.hpp with
// start = 0, ms = n and the top-row delta +1: same lanes, same systolic column loop, same [step][lane] trace store with every column
// kept.  The distance is the score of the query's last row at the last column.  What this header adds is the walk of the WHOLE path
// from the cell (m, n) -- hwf_walk returns the leading run only -- and the run-length ops it emits:
//   op = len << 4 | code, codes 0 '=', 1 'X', 2 'I' (query only), 3 'D' (target only).
// The walk follows the oracle's tie rule (Pv bit: 'I', else Ph bit: 'D', else the diagonal) and goes on along the borders: the rows
// left at column 0 are one 'I' run, the columns left at row 0 one 'D' run.  Pv / Ph do not tell '=' from 'X': the two bases do.
// Runs come out in walk order, i.e. REVERSED; nwp_forward_runs turns such a list into the forward one.
// The same header is compiled by g++ for tests/emul/nw_path_emul.cpp (64 emulated lanes in lock step, against the oracle).
#pragma once
#include "hw_full_core.hpp"

namespace isocon {

enum { NWP_EQ = 0, NWP_X = 1, NWP_I = 2, NWP_D = 3 };

ISO_HD uint32_t nwp_op(int32_t code, int32_t len) { return ((uint32_t)len << 4) | (uint32_t)code; }
ISO_HD int32_t nwp_op_code(uint32_t op) { return (int32_t)(op & 15u); }
ISO_HD uint32_t nwp_op_len(uint32_t op) { return op >> 4; }

// Runs of a path of distance ed: every run that is not '=' holds at least one edit, and '=' runs alternate with those: at most
// ed of the former, ed + 1 of the latter.  The per-pair op storage is sized from this, not from m + n.
ISO_HD uint64_t nwp_max_runs(int32_t ed) { return 2 * (uint64_t)(ed < 0 ? 0 : ed) + 1; }

// The walk from the end cell (m, n) to (0, 0).
//   load(block, j, pv, ph)   what the TRACE pass kept for column j (1-based) of the block (hwf_trace_unit)
//   same_base(i, j)          q[i - 1] == t[j - 1]; only called for the cell whose block and column the LAST load named
//   emit(code, len)          one run, maximal (adjacent runs differ, none is empty), in walk order = reversed
// Returns the number of runs.
template <class Load, class Same, class Emit>
ISO_HD int32_t nwp_walk(int32_t m, int32_t n, Load load, Same same_base, Emit emit)
{
    int32_t i = m, j = n, code = -1, len = 0, runs = 0;
    while (i > 0 && j > 0) {
        const int32_t bit = (i - 1) & 63;
        uint64_t pv, ph;
        load((i - 1) >> 6, j, pv, ph);
        int32_t c;
        if ((pv >> bit) & 1) { c = NWP_I; --i; }
        else if ((ph >> bit) & 1) { c = NWP_D; --j; }
        else { c = same_base(i, j) ? NWP_EQ : NWP_X; --i; --j; }
        if (c == code) ++len;
        else {
            if (len) { emit(code, len); ++runs; }
            code = c; len = 1;
        }
    }
    // the borders: D[i][0] = i and D[0][j] = j, so the rule gives 'I' down column 0 and 'D' along row 0
    const int32_t c = i > 0 ? NWP_I : NWP_D, rest = i > 0 ? i : j;
    if (rest > 0) {
        if (c == code) len += rest;
        else {
            if (len) { emit(code, len); ++runs; }
            code = c; len = rest;
        }
    }
    if (len) { emit(code, len); ++runs; }
    return runs;
}

// Reversed run list -> forward list: last run first, equal neighbours merged, empty runs dropped.  fwd may be nullptr (count only);
// it must not overlap rev.  Returns the number of forward runs (<= n_rev).
ISO_HD uint64_t nwp_forward_runs(const uint32_t *rev, uint64_t n_rev, uint32_t *fwd)
{
    uint64_t out = 0;
    uint32_t cur = 0;              // the run being merged (length 0: none)
    for (uint64_t a = n_rev; a-- > 0;) {
        const uint32_t op = rev[a];
        if (nwp_op_len(op) == 0) continue;
        if (nwp_op_len(cur) && nwp_op_code(cur) == nwp_op_code(op)) { cur += nwp_op_len(op) << 4; continue; }
        if (nwp_op_len(cur)) { if (fwd) fwd[out] = cur; ++out; }
        cur = op;
    }
    if (nwp_op_len(cur)) { if (fwd) fwd[out] = cur; ++out; }
    return out;
}

}  // namespace isocon
