"""The per-edge hypothesis test of the statistical-test phase: mirror of
/root/reference/modules/hypothesis_test_module.py:20-77 (`do_statistical_tests_per_edge`), :92-171
(`arrange_alignments_new_no_realign`), :217-247 (`statistical_test`), :253-329 (`raghavan_upper_pvalue_bound`) and
:331-343 (`get_correction_factor`).

For a candidate c and its reference t: align the two (semi-global, match 2, mismatch -3, gap open 3, extend 1 -- the
reference's second gap model, hypothesis_test_module.py:99,103) in both orders and keep the order with fewer differing
columns outside the end gaps; locate the variants on both sequences; count the reads (of c and of t, from their stored
alignments) that carry all of them; bound the probability of that many supporters arising from sequencing errors alone.

The reference aligns the two orders of every edge one call at a time (or one Pool task per edge); here ALL edges of a
round go to the GPU as one batch of isocon_sg_strings_batch (2 x edges alignments), everything after that is string
bookkeeping on the host as in the reference.  With base qualities (a `ccs_dict`: FASTQ input) the error probabilities
come from the qualities (functions.get_read_ccs_probabilities_c / _t): which quality a read contributes at a variant is
looked up on the same read tables, and on the device tables the lanes multiply the reads' error probabilities up as well
(isocon_readtab_probability: the host's doubles bit for bit); the logarithms and the sums stay on the host.  The bound itself
(_raghavan_from_sums: 100-digit decimals) is evaluated for all edges of a round by one isocon_raghavan_bound call, in wide fixed point
with a certificate per test that its double is float() of the decimal result; a test without it goes through _raghavan_from_sums."""
from __future__ import annotations

import collections
import ctypes
import decimal
import math
import operator
import os

import numpy as np

from . import _lib
from . import functions
from . import SW_alignment_module as SWM


# An edge's variants, where they lie on t and on c (the reference's variant_coords_t / _c), and per variant the snippet of c's row under t's
# coordinate and of t's row under c's (alignment_c_to_t / alignment_t_to_c); a query of the device tables (_pack_queries).  Equal to plain tuples.
_EdgeVariants = collections.namedtuple("_EdgeVariants", "variants coords_t coords_c c_to_t t_to_c")
_Query = collections.namedtuple("_Query", "table kind coords snippets n_rows")


# What differs between the reads of c and of t in a test (functions.get_support, get_read_ccs_probabilities_c / _t): the kind of their device queries;
# getters on an _EdgeVariants for their variant coordinates, for the snippets of a support query (none: the reads are compared with their candidate's
# row) and for the other sequence's snippets of a quality query; the variant type at which the other sequence's window lies a column to the left; by
# variant type, where a read that shows the other sequence has its judged base among the read bases seen (-1 unless listed).  _SIDES: by query kind.
_Side = collections.namedtuple("_Side", "kind coords support_snippets quality_snippets shifted_type coord_when_other")
_SIDE_C = _Side(0, operator.attrgetter("coords_c"), lambda ev: None, operator.attrgetter("t_to_c"), "D", {"I": 0})
_SIDE_T = _Side(1, operator.attrgetter("coords_t"), operator.attrgetter("c_to_t"), operator.attrgetter("c_to_t"), "I", {"D": 0, "I": -2})
_SIDES = (_SIDE_C, _SIDE_T)


def _other_window(shifted_type, v_type, u_v):
    """(columns before, columns after) a variant's position in which a read shows the other sequence's snippet"""
    return (2, u_v) if v_type == shifted_type else (1, u_v + 1)


def _clamp(a, hi):
    """a limited to [0, hi] (np.clip with less call overhead: this runs per variant and window column of every edge)"""
    return np.minimum(np.maximum(a, 0), hi)


class _ReadTable(object):
    """The stored alignments of one candidate's reads as flat arrays, so that the per-read quantities of a test --
    alignment column of a candidate position, error counts, window comparisons -- are computed once per round and for all
    reads at a time instead of once per (edge, read) as functions.get_support / get_read_errors do.  Same results
    (tests/test_stat_test.py::test_read_tables_equal_the_per_read_functions)."""

    def __init__(self, ref_len, read_alignments):
        self.__dict__.update(_build_tables([(ref_len, read_alignments)])[0].__dict__)

    def column_of(self, i, still_ok):
        """alignment column of candidate position i, per read (functions.get_support: c_seq_to_coord_in_almnt[i])"""
        if not -self.ref_len <= i < self.ref_len:
            if still_ok.any():
                raise IndexError("list index out of range")         # what the per-read statement raises for these reads
            return np.zeros(self.n, dtype=np.int64)
        if i < 0:
            i += self.ref_len
        return i + np.bincount(self.gap_row[self.gap_h <= i], minlength=self.n)

    def agree_with_candidate(self, variant_coords):
        """reads whose row equals the candidate's row over every variant window (get_support, reads of c)"""
        ok = np.ones(self.n, dtype=bool)
        for i, (_, _, u_v) in variant_coords.items():
            ok &= self.own_window_equal(self.column_of(i, ok), u_v)
        return ok

    def show_snippets(self, variant_coords, snippets):
        """reads that show the other sequence's snippet at every variant (get_support, reads of t)"""
        ok = np.ones(self.n, dtype=bool)
        for i, (v_type, _, u_v) in variant_coords.items():
            ok &= self.window_equals(self.column_of(i, ok), *_other_window(_SIDE_T.shifted_type, v_type, u_v), snippets[i])
        return ok

    # ---- pieces of the quality-based probabilities (functions._ccs_probabilities), per read and per variant ----
    def own_window_equal(self, pos, u_v):
        """aln_read[lo:hi] == aln_own[lo:hi] with lo = max(0, pos - 1), hi = pos + u_v + 1"""
        ok = np.ones(self.n, dtype=bool)
        for w in range(-1, u_v + 1):
            col = pos + w
            valid = (col >= 0) & (col < self.len)
            ok &= ~(valid & self.diff[_clamp(self.off0 + col, self.total - 1)])
        return ok

    def window_equals(self, pos, before, after, text):
        """aln_read[max(0, pos - before): pos + after] == text"""
        snippet = np.frombuffer(text.encode("ascii"), dtype=np.uint8)
        lo = np.maximum(0, pos - before)
        hi = np.minimum(self.len, pos + after)
        match = np.maximum(hi - lo, 0) == len(snippet)
        for j in range(len(snippet)):
            match &= self.read[_clamp(self.off0 + lo + j, self.total - 1)] == snippet[j]
        return match

    def read_bases_upto(self, pos):
        """number of read bases in aln_read[:pos + 1]"""
        if getattr(self, "_rgap_key", None) is None:
            g = np.flatnonzero(self.read == 45)
            row = np.searchsorted(self.off0, g, side="right") - 1
            self._rgap_key = row * (np.int64(1) << 32) + (g - self.off0[row])          # sorted: by row, then column
            self._rgap_first = np.searchsorted(row, np.arange(self.n + 1))
        rows = np.arange(self.n, dtype=np.int64)
        upto = np.searchsorted(self._rgap_key, rows * (np.int64(1) << 32) + np.clip(pos, -1, (1 << 31) - 1), side="right") - self._rgap_first[:-1]
        return pos + 1 - np.where(pos >= 0, upto, 0)

    def qualities(self, ccs_dict):
        """(flat qualities, offset of every read's record, record length, start of the read inside its record)"""
        if getattr(self, "_qual_of", None) is not ccs_dict:
            recs = [ccs_dict[acc] for acc in self.accs]          # (KeyError, and ValueError from _read_starts: the caller's)
            flat, off = _quality_arrays(recs)
            self._qual = (flat, off[:-1], np.fromiter((len(r.seq) for r in recs), dtype=np.int64, count=self.n), _read_starts(recs, self.read_rows_without_gaps()))
            self._qual_of = ccs_dict
        return self._qual

    def read_rows_without_gaps(self):
        raw = self.read.tobytes().decode("ascii")
        o = self.off0.tolist() + [self.total]
        return [raw[o[r]:o[r + 1]].replace("-", "") for r in range(self.n)]


def _quality_arrays(recs):
    """(the records' quality lists as one flat int64 array, their len(recs) + 1 offsets in it); a record keeps its array (_qual_np)"""
    for r in recs:                                  # the record's quality list as an array, made once per record
        if getattr(r, "_qual_np_of", None) is not r.qual:
            r._qual_np, r._qual_np_of = np.asarray(r.qual, dtype=np.int64), r.qual
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r._qual_np) for r in recs], out=off[1:])
    return (np.concatenate([r._qual_np for r in recs]) if recs else np.zeros(0, dtype=np.int64)), off


def _read_starts(recs, reads):
    """where each read (without gaps) starts in its record's sequence; ValueError for a record that does not hold its read"""
    return np.fromiter((r.seq.index(x) for r, x in zip(recs, reads)), dtype=np.int64, count=len(recs))


# What one read says at one variant, as a byte (csrc/readtab_core.hpp rt_quality_code): its quality 0 .. 93 there, or
_Q_INDEX, _Q_BEYOND, _Q_BOTH, _Q_NEITHER = 0xFC, 0xFD, 0xFE, 0xFF


def _quality_codes_on_table(tab, i, v_type, u_v, alive, other_snippet, ccs_dict, shifted_type, coord_when_other):
    """the code byte of every read of a host table at one variant (alive: the reads still informative, for column_of's IndexError)"""
    flat, qoff, rec_len, rec_start = tab.qualities(ccs_dict)
    pos = tab.column_of(i, alive)
    shows_own = tab.own_window_equal(pos, u_v)
    shows_other = tab.window_equals(pos, *_other_window(shifted_type, v_type, u_v), other_snippet)
    seen = tab.read_bases_upto(pos)
    read_coord = np.where(shows_own, seen - 1, seen + coord_when_other.get(v_type, -1))
    coord = rec_start + read_coord                     # CCS.read_aln_to_ccs_coord
    beyond = coord > rec_len
    coord = np.where(coord == rec_len, coord - 1, coord)
    coord = np.where(coord < 0, coord + rec_len, coord)        # a negative list index counts from the end
    outside = (coord < 0) | (coord >= rec_len)
    q = flat[np.clip(qoff + np.clip(coord, 0, np.maximum(rec_len - 1, 0)), 0, max(len(flat) - 1, 0))] if len(flat) else np.zeros(tab.n, dtype=np.int64)
    code = np.clip(q, 0, 93)
    code = np.where(outside, _Q_INDEX, code)
    code = np.where(beyond, _Q_BEYOND, code)
    code = np.where(~shows_own & ~shows_other, _Q_NEITHER, code)
    return np.where(shows_own & shows_other, _Q_BOTH, code).astype(np.uint8)


_P_OF_QUALITY = {}     # max_phred_q_trusted -> the 94 error probabilities (read-only array)


def _p_of_quality(max_phred_q_trusted):
    """the error probability of every quality value 0 .. 93 mapped onto [3, max_phred_q_trusted] (functions._ccs_probabilities:
    q_qual_mapped, 10 ** (-q_qual_mapped / 10.0)), made once per max_phred_q_trusted: the host route and the device route read the same doubles"""
    base = _P_OF_QUALITY.get(max_phred_q_trusted)
    if base is None:
        base = np.asarray([10 ** (-((q - 3) * (max_phred_q_trusted - 3.0) / (90.0) + 3) / 10.0) for q in range(94)], dtype=np.float64)
        base.setflags(write=False)
        _P_OF_QUALITY[max_phred_q_trusted] = base
    return base


def _error_ratios(tab_c, tab_t):
    """(substitution, insertion, deletion) shares of the errors of the reads of an edge (functions.get_read_ccs_probabilities_c / _t)"""
    subs = float(max(1.0, int(tab_t.sub.sum() + tab_c.sub.sum())))
    ins = float(max(1.0, int(tab_t.ins.sum() + tab_c.ins.sum())))
    del_ = float(max(1.0, int(tab_t.dele.sum() + tab_c.dele.sum())))
    tot_errors = subs + ins + del_
    return (subs / tot_errors, ins / tot_errors, del_ / tot_errors)


def _ccs_probabilities_from_codes(n, variant_coords, code_of, ratios, max_phred_q_trusted):
    """functions._ccs_probabilities for the n reads of a table at once: (informative mask, probability per read).  code_of(v, i, v_type,
    u_v, alive) gives the reads' code bytes at the v-th variant: _quality_codes_on_table on the host tables, a row of
    isocon_readtab_quality's answer on the device tables.  Every float statement of the quality route is here."""
    subs_ratio, ins_ratio, del_ratio = ratios
    assert len(variant_coords) > 0
    alive = np.ones(n, dtype=bool)
    prob = np.ones(n, dtype=np.float64)
    if n == 0:
        return alive, prob
    base = _p_of_quality(max_phred_q_trusted)
    for v, (i, (v_type, _, u_v)) in enumerate(variant_coords.items()):
        code = code_of(v, i, v_type, u_v, alive)
        assert not (alive & (code == _Q_BOTH)).any()
        alive &= code != _Q_NEITHER
        if (alive & (code == _Q_BEYOND)).any():
            raise SystemExit("Index error: read position beyond its quality record")
        if (alive & (code == _Q_INDEX)).any():
            raise IndexError("list index out of range")
        p10 = base[np.minimum(code, 93)]
        if u_v > 1:
            p_error = p10
        elif v_type == "S":
            p_error = (p10 * subs_ratio) / 3.0
        elif v_type == "I":
            p_error = (p10 * ins_ratio) / 4.0
        else:
            p_error = p10 * del_ratio
        prob = np.where(alive, prob * p_error, prob)
    assert ((prob[alive] > 0.0) & (prob[alive] < 1.0)).all()
    return alive, prob


def _ccs_probabilities_on_table(side, work, ev, ccs_dict, ratios, max_phred_q_trusted):
    """_ccs_probabilities_from_codes for the table of one side (work: its _SideWork) of the edge ev: a device table brings the finished products
    (_device_probability's answer: one double per read, negative = not informative) or its codes (_device_quality's), a host table computes its codes"""
    if work.probs is not None:
        alive = work.probs >= 0
        assert ((work.probs[alive] > 0.0) & (work.probs[alive] < 1.0)).all()
        return alive, work.probs
    tab, codes, variant_coords, other_snippets = work.tab, work.codes, side.coords(ev), side.quality_snippets(ev)
    if codes is not None:
        return _ccs_probabilities_from_codes(tab.n, variant_coords, lambda v, i, v_type, u_v, alive: codes[v], ratios, max_phred_q_trusted)
    return _ccs_probabilities_from_codes(tab.n, variant_coords, lambda v, i, v_type, u_v, alive: _quality_codes_on_table(
        tab, i, v_type, u_v, alive, other_snippets[i], ccs_dict, side.shifted_type, side.coord_when_other), ratios, max_phred_q_trusted)


def _variants_of(aln_t, aln_c):
    start, end = functions.get_mask_start_and_end(aln_t, aln_c)           # indels in the ends are length differences, not variants
    a = np.frombuffer(aln_t.encode("ascii"), dtype=np.uint8)
    b = np.frombuffer(aln_c.encode("ascii"), dtype=np.uint8)
    return [(i, aln_t[i], aln_c[i]) for i in np.flatnonzero(a != b).tolist() if start <= i < end]


def _candidate_vs_reference(alignment_tc, alignment_ct):
    """hypothesis_test_module.py:99-110: (aln_t, aln_c, variants) from the t-vs-c alignment unless the c-vs-t alignment has
    strictly fewer variants."""
    aln_t, aln_c = alignment_tc[0], alignment_tc[1]
    variants = _variants_of(aln_t, aln_c)
    aln_c_flip, aln_t_flip = alignment_ct[0], alignment_ct[1]
    variants_flipped = _variants_of(aln_t_flip, aln_c_flip)
    if len(variants_flipped) < len(variants):
        return aln_t_flip, aln_c_flip, variants_flipped
    return aln_t, aln_c, variants


def _test_on_alignments(t_seq, c_seq, alignment_tc, alignment_ct, read_alignments_to_c, read_alignments_to_t, ccs_dict=None, max_phred_q_trusted=None):
    """hypothesis_test_module.py:92-171 after the two alignments: (variant_coords_t, p_value, supporting reads, reads used)."""
    aln_t, aln_c, variants = _candidate_vs_reference(alignment_tc, alignment_ct)
    variant_coords_t, variant_coords_c, alignment_c_to_t, alignment_t_to_c = functions.get_variant_coordinates(t_seq, c_seq, aln_t, aln_c, variants)
    reads_support = functions.get_support(read_alignments_to_c, variant_coords_c, read_alignments_to_t, variant_coords_t, alignment_c_to_t)
    if len(variants) == 0:      # identical up to the ignored ends
        return variant_coords_t, 0.0, reads_support, len(read_alignments_to_c) + len(read_alignments_to_t)
    errors = functions.get_read_errors(read_alignments_to_c, read_alignments_to_t)
    if ccs_dict:            # base qualities decide (FASTQ input): reads showing neither sequence at a variant drop out
        probability, _ = functions.get_read_ccs_probabilities_c(read_alignments_to_c, variant_coords_c, alignment_t_to_c, ccs_dict, errors, max_phred_q_trusted)
        probability.update(functions.get_read_ccs_probabilities_t(read_alignments_to_t, variant_coords_t, alignment_c_to_t, ccs_dict, errors, max_phred_q_trusted)[0])
    else:
        probability = functions.get_empirical_error_probabilities(len(t_seq), errors, variant_coords_t)
    if len(probability) == 0:
        assert len(reads_support) == 0
        p_value = 0.0
    else:
        p_value = raghavan_upper_pvalue_bound(probability, reads_support)
    return variant_coords_t, p_value, reads_support, len(probability)


def _build_tables(items):
    """_ReadTable objects for [(ref_len, read_alignments)]: one pass of array operations over the reads of all of them,
    the tables are slices of the shared arrays."""
    per, rows_ref, rows_read, end_ref, end_read = [0], [], [], [], []
    for _, ra in items:
        for v in ra.values():
            a, b = v[0], v[1]
            rows_ref.append(a)
            rows_read.append(b)
            # columns of the leading + trailing gap run of either row (they are not errors: read_errors_from_alignment)
            end_ref.append(2 * len(a) - len(a.lstrip("-")) - len(a.rstrip("-")))
            end_read.append(2 * len(b) - len(b.lstrip("-")) - len(b.rstrip("-")))
        per.append(len(rows_ref))
    n = len(rows_ref)
    lens = np.fromiter((len(r) for r in rows_ref), dtype=np.int64, count=n)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    off0 = off[:-1]
    ref = np.frombuffer("".join(rows_ref).encode("ascii"), dtype=np.uint8)
    read = np.frombuffer("".join(rows_read).encode("ascii"), dtype=np.uint8)
    diff = ref != read
    # gaps of the candidate's row: a gap with h candidate characters before it shifts every position >= h by one column
    g = np.flatnonzero(ref == 45)
    gap_row = np.searchsorted(off, g, side="right") - 1
    first_gap = np.searchsorted(gap_row, np.arange(n + 1))
    gap_h = (g - off0[gap_row]) - (np.arange(len(g), dtype=np.int64) - first_gap[gap_row])
    # Error counts between the end gaps (functions.read_errors_from_alignment).  A column never holds two gaps and an end
    # run of one row faces bases of the other, so: insertions = gaps of the candidate's row outside its end runs,
    # deletions = the same for the read's row, substitutions = the remaining differing columns.
    if n:
        gaps_ref = first_gap[1:] - first_gap[:-1]
        gaps_read = np.fromiter((r.count("-") for r in rows_read), dtype=np.int64, count=n)
        ins = gaps_ref - np.asarray(end_ref, dtype=np.int64)
        dele = gaps_read - np.asarray(end_read, dtype=np.int64)
        sub = np.add.reduceat(diff.view(np.uint8), off0, dtype=np.int64) - gaps_ref - gaps_read
    else:
        ins = dele = sub = np.zeros(0, dtype=np.int64)
    tables = []
    for k, (ref_len, ra) in enumerate(items):
        r0, r1 = per[k], per[k + 1]
        b0, b1 = int(off[r0]), int(off[r1])
        g0, g1 = int(first_gap[r0]), int(first_gap[r1])
        t = _ReadTable.__new__(_ReadTable)
        t.accs = list(ra)
        t.n = r1 - r0
        t.ref_len = ref_len
        t.len = lens[r0:r1]
        t.off0 = off0[r0:r1] - b0
        t.total = b1 - b0
        t.read = read[b0:b1]
        t.diff = diff[b0:b1]
        t.gap_row = gap_row[g0:g1] - r0
        t.gap_h = gap_h[g0:g1]
        t.ins, t.dele, t.sub = ins[r0:r1], dele[r0:r1], sub[r0:r1]
        tables.append(t)
    return tables


_TABLES = {}        # id(read-alignment dict) -> (the dict, its alignment tuples, table); reset by clear_tables()
_DEVICE_TABLES = {}     # the same for the tables kept on the device (_DeviceTable)


def _device_sets():
    """the table sets (_DeviceSet) of the cached device tables, each once"""
    return {id(hit[2].set): hit[2].set for hit in _DEVICE_TABLES.values()}.values()


def clear_tables():
    _TABLES.clear()
    for dset in _device_sets():
        dset.free()
    _DEVICE_TABLES.clear()


def _tables_for(wanted, cache=None, build=None):
    """{id(read_alignments): table} for [(ref_seq, read_alignments)]; a table is rebuilt only when the candidate's reads or
    their alignments have changed since the last round (the loop keeps most partitions untouched from round to round).
    cache / build: the host tables (_TABLES, _build_tables) unless given."""
    cache = _TABLES if cache is None else cache
    build = _build_tables if build is None else build
    out, todo = {}, []
    for ref_seq, ra in wanted:
        if id(ra) in out:
            continue
        stamp = list(ra.values())           # the alignment tuples themselves (kept alive: identities cannot be recycled)
        hit = cache.get(id(ra))
        if (hit is not None and hit[0] is ra and len(hit[1]) == len(stamp) and all(a is b for a, b in zip(hit[1], stamp))
                and hit[2].ref_len == len(ref_seq)):
            out[id(ra)] = hit[2]
        else:
            out[id(ra)] = None
            todo.append((ref_seq, ra, stamp))
    if len(cache) > 200000:
        cache.clear()          # (a device set goes with its last table)
    for lo in range(0, len(todo), 2048):                 # bounded batches: the shared arrays stay small
        part = todo[lo:lo + 2048]
        for (ref_seq, ra, stamp), tab in zip(part, build([(len(r), a) for r, a, _ in part])):
            cache[id(ra)] = (ra, stamp, tab)
            out[id(ra)] = tab
    return out


# ---- the read tables on the device (isocon_readtab_*: csrc/readtab.hpp) ----
# The integer work of a test -- the column of a candidate position in every read's alignment, the window comparisons, the error
# counts -- for all edges of a round in one call per table set, and with base qualities every read's error probability over the variants
# of its edge; the logarithms and the sums stay on the host (_test_on_supporters), the bounds of the round follow in one call (_device_bounds).
# quality_calls: one per table set and round whose quality queries were answered (by either entry; a codes call for an edge that raises
# counts too), probability_calls: the calls of isocon_readtab_probability
DEVICE_STATS = {"create_calls": 0, "rows_uploaded": 0, "support_calls": 0, "queries": 0, "quality_attach_calls": 0, "quality_calls": 0, "probability_calls": 0,
                "kernel_ms": 0.0}
_HAS_DEVICE = None
_Routes = collections.namedtuple("_Routes", "tables variants probabilities bounds")


def _routes():
    """Which parts of a round run on the device, from ISOCON_DEBUG_VARIANT (name[=value],name,...) and the device count, for a round to ask
    once; what each switch means stands with the *_enabled() function over it below."""
    global _HAS_DEVICE
    listed = {item.split("=")[0] for item in os.environ.get("ISOCON_DEBUG_VARIANT", "").split(",")}
    if _HAS_DEVICE is None and "stat_host_tables" not in listed:
        _HAS_DEVICE = _lib.load().isocon_device_count() > 0
    tables = "stat_host_tables" not in listed and _HAS_DEVICE
    return _Routes(tables, *(tables and name not in listed for name in ("stat_host_variants", "stat_host_prob", "stat_host_bound")))


def device_tables_enabled():
    """the tests of a round go through the device tables: a GPU is there and ISOCON_DEBUG_VARIANT=stat_host_tables is not set"""
    return _routes().tables


def edge_variants_on_device_enabled():
    """the variants of a round's edges come from the device (isocon_edge_variants): the device tables are on and stat_host_variants is not set"""
    return _routes().variants


def probabilities_on_device_enabled():
    """with base qualities the reads' probabilities come from isocon_readtab_probability, not from the code bytes: the device tables are on and stat_host_prob is not set"""
    return _routes().probabilities


def bounds_on_device_enabled():
    """the bounds of a round's tests come from the device (isocon_raghavan_bound): the device tables are on and stat_host_bound is not set"""
    return _routes().bounds


def device_table_bytes():
    """device memory held by the cached table sets"""
    return sum(s.bytes for s in _device_sets())


def _ptr(a, typ):
    return a.ctypes.data_as(typ)


class _DeviceSet(object):
    """One isocon_readtab handle: the tables of up to 2048 candidates.  Freed by clear_tables(), or with its last table."""

    def __init__(self, handle, accs=(), read_rows=()):
        self.handle = handle
        self.bytes = int(_lib.lib().isocon_readtab_device_bytes(handle))
        self.accs, self.read_rows = accs, read_rows          # per row: the read's accession and its gapped row (the stored string itself)
        self.qual_of, self.qual_ok = None, False             # the ccs_dict whose qualities are attached; False: they cannot be (host tables)

    def attach_qualities(self, ccs_dict):
        """the base qualities of the set's reads (ccs_dict[acc].qual) onto the device, once per ccs_dict: one isocon_readtab_set_qualities.
        Returns False -- the set's edges then go through the host tables, which raise what there is to raise -- when a record is
        missing, does not hold its read, or does not have one quality 0 .. 93 per base."""
        if self.qual_of is ccs_dict:
            return self.qual_ok
        self.qual_of, self.qual_ok = ccs_dict, False
        n = len(self.accs)
        try:
            recs = [ccs_dict[acc] for acc in self.accs]
            start = _read_starts(recs, [row.replace("-", "") for row in self.read_rows])
        except (KeyError, ValueError):
            return False
        flat, off = _quality_arrays(recs)
        if any(len(r.seq) != len(r._qual_np) for r in recs):
            return False
        if len(flat) and (flat.min() < 0 or flat.max() > 93):
            return False
        qual = flat.astype(np.uint8) if len(flat) else np.zeros(1, dtype=np.uint8)
        qual_ptr = off.astype(np.uint64)
        rec_start = start.astype(np.uint32) if n else np.zeros(1, dtype=np.uint32)
        ms = ctypes.c_float(0.0)
        _lib.check(_lib.lib().isocon_readtab_set_qualities(self.handle, _ptr(qual, _lib.u8p), _ptr(qual_ptr, _lib.u64p), _ptr(rec_start, _lib.u32p), ctypes.byref(ms)),
                   "isocon_readtab_set_qualities")
        DEVICE_STATS["quality_attach_calls"] += 1
        DEVICE_STATS["kernel_ms"] += ms.value
        self.bytes = int(_lib.lib().isocon_readtab_device_bytes(self.handle))
        self.qual_ok = True
        return True

    def free(self):
        if self.handle is not None:
            _lib.lib().isocon_readtab_destroy(self.handle)
            self.handle, self.bytes = None, 0
            self.qual_of, self.qual_ok = None, False

    def __del__(self):
        try:
            self.free()
        except Exception:          # (interpreter shutdown)
            pass


class _DeviceTable(object):
    """table k of a set: what _test_on_supporters needs on the host (sizes and error counts), the rest lives in the set"""
    __slots__ = ("set", "k", "n", "ref_len", "ins", "dele", "sub", "accs")


def _pack_rows(items):
    """the rows of [(ref_len, read_alignments)] as isocon_readtab_create takes them: (candidate rows, read rows, row_ptr, first_row)"""
    rows_ref, rows_read, first_row = [], [], [0]
    for _, ra in items:
        for v in ra.values():
            if len(v[0]) != len(v[1]):
                raise ValueError("the two rows of a read alignment differ in length")
            rows_ref.append(v[0])
            rows_read.append(v[1])
        first_row.append(len(rows_ref))
    n = len(rows_ref)
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(r) for r in rows_ref), dtype=np.uint64, count=n), out=row_ptr[1:])
    ref = np.frombuffer("".join(rows_ref).encode("ascii"), dtype=np.uint8)
    read = np.frombuffer("".join(rows_read).encode("ascii"), dtype=np.uint8)
    return ref, read, row_ptr, np.asarray(first_row, dtype=np.uint32)


def _build_device_tables(items):
    """_DeviceTable objects for [(ref_len, read_alignments)]: one table set"""
    L = _lib.lib()
    ref, read, row_ptr, first_row = _pack_rows(items)
    n = len(row_ptr) - 1
    errors = np.zeros((max(n, 1), 3), dtype=np.uint32)
    handle, ms = ctypes.c_void_p(), ctypes.c_float(0.0)
    _lib.check(L.isocon_readtab_create(_ptr(ref, _lib.u8p), _ptr(read, _lib.u8p), _ptr(row_ptr, _lib.u64p), n, _ptr(first_row, _lib.u32p), len(items),
                                       ctypes.byref(handle), _ptr(errors, _lib.u32p), ctypes.byref(ms)), "isocon_readtab_create")
    DEVICE_STATS["create_calls"] += 1
    DEVICE_STATS["rows_uploaded"] += n
    DEVICE_STATS["kernel_ms"] += ms.value
    dset = _DeviceSet(handle, [acc for _, ra in items for acc in ra], [v[1] for _, ra in items for v in ra.values()])
    errors = errors[:n].astype(np.int64)
    tables = []
    for k, (ref_len, _) in enumerate(items):
        r0, r1 = int(first_row[k]), int(first_row[k + 1])
        t = _DeviceTable()
        t.set, t.k, t.n, t.ref_len = dset, k, r1 - r0, ref_len
        t.accs = dset.accs[r0:r1]
        t.ins, t.dele, t.sub = errors[r0:r1, 0], errors[r0:r1, 1], errors[r0:r1, 2]
        tables.append(t)
    return tables


def _pack_queries(queries):
    """[(table index, kind, variant_coords, snippets or None, rows of the table)] as isocon_readtab_support / _quality take them: (q_table,
    q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, bits_ptr)"""
    q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_len, snips, bits_ptr = [], [], [0], [], [], [], [], [], [0]
    for k, kind, coords, snippets, n_rows in queries:
        q_table.append(k)
        q_kind.append(kind)
        for i, (v_type, _, u_v) in coords.items():
            var_pos.append(i)
            var_u.append(u_v)
            var_type.append(ord(v_type))
            text = snippets[i] if snippets is not None else ""
            snips.append(text)
            snip_len.append(len(text))
        var_ptr.append(len(var_pos))
        bits_ptr.append(bits_ptr[-1] + (n_rows + 63) // 64)
    snip_ptr = np.zeros(len(snip_len) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(snip_len, dtype=np.uint64), out=snip_ptr[1:])
    snip_bytes = np.frombuffer("".join(snips).encode("ascii"), dtype=np.uint8)
    if len(snip_bytes) == 0:
        snip_bytes = np.zeros(1, dtype=np.uint8)
    return (np.asarray(q_table, dtype=np.uint32), np.asarray(q_kind, dtype=np.uint8), np.asarray(var_ptr, dtype=np.uint64),
            np.asarray(var_pos, dtype=np.int32), np.asarray(var_u, dtype=np.int32), np.asarray(var_type, dtype=np.uint8), snip_ptr, snip_bytes,
            np.asarray(bits_ptr, dtype=np.uint64))


def _rows_of_bits(words, n_rows):
    """indices of the set bits among the first n_rows of a bit set (uint64 words, bit j of word j // 64)"""
    return np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows])


def _query_call(entry, handle, packed, *own):
    """one call of a query entry of the device tables (isocon_readtab_support / _quality / _probability): the set, the number of queries and
    q_table .. snip_bytes of _pack_queries, which all three take alike, then the entry's own arrays as (array, pointer type); adds the kernel time"""
    shared = zip(packed, (_lib.u32p, _lib.u8p, _lib.u64p, _lib.i32p, _lib.i32p, _lib.u8p, _lib.u64p, _lib.u8p))
    ms = ctypes.c_float(0.0)
    _lib.check(getattr(_lib.lib(), entry)(handle, len(packed[0]), *[_ptr(a, t) for a, t in list(shared) + list(own)], ctypes.byref(ms)), entry)
    DEVICE_STATS["kernel_ms"] += ms.value


def _device_support(handle, queries):
    """one isocon_readtab_support call: the supporting rows (ascending indices into its table) of every query of _pack_queries"""
    if not queries:
        return []
    packed = _pack_queries(queries)
    bits_ptr = packed[8]
    bits = np.zeros(max(int(bits_ptr[-1]), 1), dtype=np.uint64)
    count = np.zeros(len(queries), dtype=np.uint32)
    _query_call("isocon_readtab_support", handle, packed, (bits_ptr, _lib.u64p), (bits, _lib.u64p), (count, _lib.u32p))
    DEVICE_STATS["support_calls"] += 1
    DEVICE_STATS["queries"] += len(queries)
    out = []
    for q, (_, _, _, _, n_rows) in enumerate(queries):
        sup = _rows_of_bits(bits[int(bits_ptr[q]):int(bits_ptr[q + 1])], n_rows) if count[q] else np.zeros(0, dtype=np.int64)
        assert len(sup) == int(count[q])
        out.append(sup)
    return out


def _device_quality(handle, queries):
    """one isocon_readtab_quality call: the code bytes (variants x rows, uint8) of every query of _pack_queries (snippets for both kinds)"""
    if not queries:
        return []
    code_ptr = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum(np.asarray([len(coords) * n_rows for _, _, coords, _, n_rows in queries], dtype=np.uint64), out=code_ptr[1:])
    codes = np.zeros(max(int(code_ptr[-1]), 1), dtype=np.uint8)
    _query_call("isocon_readtab_quality", handle, _pack_queries(queries), (code_ptr, _lib.u64p), (codes, _lib.u8p))
    DEVICE_STATS["quality_calls"] += 1
    return [codes[int(code_ptr[q]):int(code_ptr[q + 1])].reshape(len(coords), n_rows) for q, (_, _, coords, _, n_rows) in enumerate(queries)]


PROBABILITY_CALL_BYTES = 256 << 20          # a set's queries are split over several calls only if their doubles exceed this


def _device_probability(handle, queries, ratios, max_phred_q_trusted):
    """isocon_readtab_probability for the queries of _pack_queries (snippets for both kinds; ratios: per query the edge's _error_ratios):
    per query (float64 per row of its table -- the read's probability, -1.0 where it is not informative --, status); a status other
    than 0 says what the codes route raises for this query: (variant index + 1) << 8 | code byte.  One call unless the answers exceed
    PROBABILITY_CALL_BYTES."""
    out, lo = [], 0
    while lo < len(queries):
        hi, rows = lo + 1, queries[lo][4]
        while hi < len(queries) and (rows + queries[hi][4]) * 8 <= PROBABILITY_CALL_BYTES:
            rows += queries[hi][4]
            hi += 1
        prob_ptr = np.zeros(hi - lo + 1, dtype=np.uint64)
        np.cumsum(np.asarray([query[4] for query in queries[lo:hi]], dtype=np.uint64), out=prob_ptr[1:])
        probs = np.zeros(max(int(prob_ptr[-1]), 1), dtype=np.float64)
        status = np.zeros(hi - lo, dtype=np.uint32)
        q_ratios = np.ascontiguousarray(ratios[lo:hi], dtype=np.float64).reshape(hi - lo, 3)
        _query_call("isocon_readtab_probability", handle, _pack_queries(queries[lo:hi]), (q_ratios, _lib.f64p), (_p_of_quality(max_phred_q_trusted), _lib.f64p),
                    (prob_ptr, _lib.u64p), (probs, _lib.f64p), (status, _lib.u32p))
        DEVICE_STATS["probability_calls"] += 1
        ptr = prob_ptr.tolist()
        out.extend((probs[ptr[q]:ptr[q + 1]], s) for q, s in enumerate(status.tolist()))
        lo = hi
    return out


def _in_range(coords, ref_len):
    return all(-ref_len <= i < ref_len for i in coords)


class _SideWork(object):
    """One side of one edge through a round -- the reads of c, or of t: their table (host or device) and the supporting rows (ascending
    indices into it).  On the device tables also its queries (quality_query and the edge's ratios: None where the test looks at no quality)
    and what the device said about the qualities: probs and status (_device_probability) or codes (_device_quality); neither: a host table computes its own."""
    __slots__ = ("tab", "supporters", "codes", "probs", "status", "support_query", "quality_query", "ratios")

    def __init__(self, tab, supporters=None, codes=None, probs=None):
        self.tab, self.supporters, self.codes, self.probs = tab, supporters, codes, probs
        self.status = self.support_query = self.quality_query = self.ratios = None


def _tests_on_device(live, of_edge, C, read_partition, ccs_dict=None, max_phred_q_trusted=None, variants_of=None, routes=None, at=None):
    """{edge: (variant_coords_t, p_value, supporting reads, reads used)} for the edges of a round: supporters and error counts from the device tables, one
    support call per table set; with base qualities (ccs_dict) also every read's probability (or, under ISOCON_DEBUG_VARIANT=stat_host_prob, its quality
    code at every variant for the host to multiply up), one call per table set. An edge for which the device reports that something is to be raised goes
    through the codes, where it is raised. An edge with a variant coordinate that the per-read statement cannot index stays on the host tables, where it
    raises; so does an edge of a table set whose qualities cannot be attached. variants_of: {edge: its _edge_variants} where the caller has them
    (_edge_variants_on_device); of_edge[e], the two gapped alignments, is then looked at only for the edges that stay on the host tables
    (_LazyAlignments). The bounds of these edges follow in one call after their loop (_resolve_bounds) if routes, the round's _routes(), says so.
    at: a one-element list that names the edge at work (None during a call for a whole batch), for a caller that has to know whose test raised."""
    routes = _routes() if routes is None else routes
    at = [None] if at is None else at
    prepared, on_host = {}, []
    for e in live:
        at[0] = e
        c_acc, t_acc = e
        ev = variants_of[e] if variants_of is not None else _edge_variants(C[t_acc], C[c_acc], of_edge[e][0], of_edge[e][1])
        ev = ev if type(ev) is _EdgeVariants else _EdgeVariants._make(ev)          # (a plain tuple from a caller of its own)
        if _in_range(ev.coords_c, len(C[c_acc])) and _in_range(ev.coords_t, len(C[t_acc])):
            prepared[e] = ev
        else:
            on_host.append(e)
    at[0] = None
    tables = _tables_for([(C[acc], read_partition[acc]) for e in prepared for acc in e], _DEVICE_TABLES, _build_device_tables)
    on_device_prob = bool(ccs_dict) and routes.probabilities
    work, by_set = {}, {}          # edge -> (its variants, its c side, its t side); id(table set) -> the sides on it, in edge order
    for e, ev in prepared.items():
        at[0] = e
        sides = [_SideWork(tables[id(read_partition[acc])]) for acc in e]
        if ccs_dict and not all(item.tab.set.attach_qualities(ccs_dict) for item in sides):
            on_host.append(e)
            continue
        work[e] = (ev, sides[0], sides[1])
        with_qualities = bool(ccs_dict) and len(ev.variants) > 0          # (no variants: the test looks at no quality)
        ratios = _error_ratios(sides[0].tab, sides[1].tab) if on_device_prob and with_qualities else None
        for side, item in zip(_SIDES, sides):
            tab, coords = item.tab, side.coords(ev)
            item.support_query = _Query(tab.k, side.kind, coords, side.support_snippets(ev), tab.n)
            if with_qualities:
                item.quality_query, item.ratios = _Query(tab.k, side.kind, coords, side.quality_snippets(ev), tab.n), ratios
            by_set.setdefault(id(item.tab.set), []).append(item)
    at[0] = None
    for batch in by_set.values():
        handle = batch[0].tab.set.handle
        for item, sup in zip(batch, _device_support(handle, [item.support_query for item in batch])):
            item.supporters = sup
        asking = [item for item in batch if item.quality_query is not None]
        queries = [item.quality_query for item in asking]
        if on_device_prob and asking:
            for item, (probs, status) in zip(asking, _device_probability(handle, queries, [item.ratios for item in asking], max_phred_q_trusted)):
                item.probs, item.status = probs, status
            DEVICE_STATS["quality_calls"] += 1
        else:
            for item, codes in zip(asking, _device_quality(handle, queries)):
                item.codes = codes
    results = {}
    pending = [] if routes.bounds else None          # (m_sum, y_sum) of the tests whose bound is still to come: the p-values are then _PendingBound
    try:
        for e, (ev, work_c, work_t) in work.items():          # (in edge order)
            at[0] = e
            if work_c.status or work_t.status:
                # something is to be raised on this edge: its code bytes, and the host's loop over them raises it (c's reads before t's)
                for item in (work_c, work_t):
                    item.codes, item.probs = _device_quality(item.tab.set.handle, [item.quality_query])[0], None
            results[e] = _test_on_supporters(C[e[1]], ev, work_c, work_t, ccs_dict, max_phred_q_trusted, pending)
    except (Exception, SystemExit):          # (what the tests themselves raise -- SystemExit is one of them --, not an interrupt)
        raised_at = at[0]
        _resolve_bounds(results, pending, at)          # the bound of an earlier edge that is to raise raises first, as it did
        at[0] = raised_at
        raise
    _resolve_bounds(results, pending, at)
    if on_host:
        host = _tables_for([(C[acc], read_partition[acc]) for e in on_host for acc in e])
        for e in on_host:
            at[0] = e
            results[e] = _test_on_tables(C[e[1]], C[e[0]], of_edge[e][0], of_edge[e][1], host[id(read_partition[e[0]])], host[id(read_partition[e[1]])],
                                         ccs_dict, max_phred_q_trusted)
    return results


# ---- Raghavan's bound on the device (isocon_raghavan_bound: csrc/pbound.hpp) ----
# _raghavan_from_sums of all tests of a round in one call.  A lane returns a double only with the certificate that it is float() of the
# 100-digit result (csrc/pbound_core.hpp); every other test -- sums outside the certified domain, where the decimals raise or
# lose digits -- is evaluated by _raghavan_from_sums itself, in edge order.
# tests: the pairs sent, certified: those that came back with the certificate, host_fallbacks: the tests then evaluated on the host
BOUND_STATS = {"calls": 0, "tests": 0, "certified": 0, "host_fallbacks": 0, "kernel_ms": 0.0}
BOUND_CALL_BYTES = 256 << 20          # the tests of a round are split over several calls only if their sums and answers exceed this


class _PendingBound(object):
    """stands in a test's tuple for the p-value that _resolve_bounds fills in: entry `at` of the round's collector"""
    __slots__ = ("at",)

    def __init__(self, at):
        self.at = at


def _device_bounds(m_sums, y_sums):
    """one isocon_raghavan_bound call: (bounds float64, certified bool) for the tests' two sums; where certified, the bound has the bits of
    _raghavan_from_sums(m_sum, y_sum), elsewhere it is 0.0"""
    m = np.ascontiguousarray(m_sums, dtype=np.float64)
    y = np.ascontiguousarray(y_sums, dtype=np.float64)
    assert m.ndim == 1 and m.shape == y.shape
    n = len(m)
    bounds, certified = np.zeros(max(n, 1), dtype=np.float64), np.zeros(max(n, 1), dtype=np.uint8)
    ms = ctypes.c_float(0.0)
    _lib.check(_lib.lib().isocon_raghavan_bound(_ptr(m, _lib.f64p), _ptr(y, _lib.f64p), n, _ptr(bounds, _lib.f64p), _ptr(certified, _lib.u8p), ctypes.byref(ms)),
               "isocon_raghavan_bound")
    certified = certified[:n] != 0
    BOUND_STATS["calls"] += 1
    BOUND_STATS["tests"] += n
    BOUND_STATS["certified"] += int(certified.sum())
    BOUND_STATS["kernel_ms"] += ms.value
    return bounds[:n], certified


def _resolve_bounds(results, pending, at=None):
    """the _PendingBound of every test in `results` replaced by its p-value: one _device_bounds call for the collector (several only above
    BOUND_CALL_BYTES), then _raghavan_from_sums for the tests that came back without a certificate, in the order of `results`.  at: as in _tests_on_device"""
    if not pending:
        return
    at = [None] if at is None else at
    at[0] = None
    per_call = max(1, BOUND_CALL_BYTES // 25)          # (16 bytes up, 9 bytes down per test)
    bounds, certified = [], []
    for lo in range(0, len(pending), per_call):
        part = pending[lo:lo + per_call]
        b, c = _device_bounds([float(m) for m, _ in part], [float(y) for _, y in part])
        bounds.extend(b.tolist())
        certified.extend(c.tolist())
    for e, (variant_coords_t, p_value, n_support, used) in results.items():
        if isinstance(p_value, _PendingBound):
            if certified[p_value.at]:
                p_value = bounds[p_value.at]
            else:
                BOUND_STATS["host_fallbacks"] += 1
                at[0] = e
                p_value = _raghavan_from_sums(*pending[p_value.at])
            results[e] = (variant_coords_t, p_value, n_support, used)
    del pending[:]


# ---- the variants of the edges on the device (isocon_edge_variants: csrc/edgevar.hpp) ----
# The candidate-vs-candidate alignments of a round stay run-length ops: which columns are variants, where they lie on t and on c, u_v and the
# snippets come from one call per round (per EDGE_VARIANT_BATCH edges); the gapped strings of an edge are made only if something asks.
EDGE_VARIANT_STATS = {"calls": 0, "edges": 0, "kernel_ms": 0.0, "lazy_expansions": 0}
EDGE_VARIANT_BATCH = 4096


class _LazyAlignments(object):
    """of_edge for a round whose alignments are ops: e -> ((aln_t, aln_c), (aln_c, aln_t)) of the (t, c) and the (c, t) alignment, expanded
    when asked for (EDGE_VARIANT_STATS["lazy_expansions"] counts the edges)"""

    def __init__(self, live, C, ops, ops_ptr):
        self._at = {e: k for k, e in enumerate(live)}
        self._C, self._ops, self._ptr, self._made = C, ops, ops_ptr, {}

    def __contains__(self, e):
        return e in self._at

    def __getitem__(self, e):
        hit = self._made.get(e)
        if hit is None:
            k, (c_acc, t_acc) = self._at[e], e
            p = self._ptr[2 * k:2 * k + 3].tolist()
            hit = self._made[e] = (SWM._ops_to_alignment(self._ops[p[0]:p[1]].tolist(), self._C[t_acc], self._C[c_acc]),
                                   SWM._ops_to_alignment(self._ops[p[1]:p[2]].tolist(), self._C[c_acc], self._C[t_acc]))
            EDGE_VARIANT_STATS["lazy_expansions"] += 1
        return hit


def _file_variant_records(rows):
    """_EdgeVariants (variants, variant_coords_t, variant_coords_c, alignment_c_to_t, alignment_t_to_c) from an edge's variant records in column order, each
    (i, key on t, key on c, u_v, type, p_t, p_c, snippet of aln_c, snippet of aln_t): filing every record under its keys in that order is
    the reference's loop (functions.get_variant_coordinates) -- a later variant on the same key overwrites the entry and keeps the key's place"""
    variants, variant_coords_t, variant_coords_c, alignment_c_to_t, alignment_t_to_c = [], {}, {}, {}, {}
    for i, key_t, key_c, u_v, v_type, p_t, p_c, snip_c, snip_t in rows:
        variants.append((i, p_t, p_c))
        entry = (v_type, p_c, u_v)
        variant_coords_t[key_t] = entry
        variant_coords_c[key_c] = entry
        alignment_c_to_t[key_t] = snip_c
        alignment_t_to_c[key_c] = snip_t
    return _EdgeVariants(variants, variant_coords_t, variant_coords_c, alignment_c_to_t, alignment_t_to_c)


def _edge_variant_capacities(ops, ops_ptr):
    """record slots an edge needs at most: the larger of its two lists' columns of ops other than '=' (ops_ptr: 2 n + 1 offsets into ops)"""
    ops = np.asarray(ops, dtype=np.uint32)
    ptr = np.asarray(ops_ptr, dtype=np.int64)
    cols = np.where((ops & 15) != 0, ops >> 4, 0).astype(np.int64)
    before = np.zeros(len(cols) + 1, dtype=np.int64)
    np.cumsum(cols, out=before[1:])
    per_list = before[ptr[1:]] - before[ptr[:-1]]
    return np.maximum(per_list[0::2], per_list[1::2])


def _edge_variants_call(seqs, edge_t, edge_c, ops, ops_ptr, rec_ptr=None):
    """one isocon_edge_variants call on plain arrays (seqs: the sequences as str; ops_ptr: 2 n + 1 offsets into ops): (flipped, n_var, bad,
    records (slots, 8) int32, snip_ptr, snippets of aln_c as str, snippets of aln_t as str, rec_ptr)"""
    n = len(edge_t)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    ops_ptr = np.ascontiguousarray(ops_ptr, dtype=np.uint64)
    if rec_ptr is None:
        rec_ptr = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(_edge_variant_capacities(ops, ops_ptr), out=rec_ptr[1:])
    rec_ptr = np.ascontiguousarray(rec_ptr, dtype=np.uint64)
    seq_ptr = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(x) for x in seqs), dtype=np.uint64, count=len(seqs)), out=seq_ptr[1:])
    seq_bytes = np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)
    if len(seq_bytes) == 0:
        seq_bytes = np.zeros(1, dtype=np.uint8)
    edge_t = np.ascontiguousarray(edge_t, dtype=np.uint32)
    edge_c = np.ascontiguousarray(edge_c, dtype=np.uint32)
    n_slots = int(rec_ptr[n] - rec_ptr[0]) if n else 0
    flipped, bad, n_var = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32)
    recs = np.zeros((max(n_slots, 1), 8), dtype=np.int32)
    snip_ptr = np.zeros(n_slots + 1, dtype=np.uint64)
    cap = 8 * n_slots + 64          # (a snippet is u_v + 2 columns; a too-small guess means running the call again)
    needed, ms = ctypes.c_uint64(0), ctypes.c_float(0.0)
    while True:
        snip_c, snip_t = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
        rc = _lib.lib().isocon_edge_variants(_ptr(seq_bytes, _lib.u8p), _ptr(seq_ptr, _lib.u64p), len(seqs), n, _ptr(edge_t, _lib.u32p), _ptr(edge_c, _lib.u32p),
                                             _ptr(ops if len(ops) else np.zeros(1, dtype=np.uint32), _lib.u32p), _ptr(ops_ptr, _lib.u64p), _ptr(rec_ptr, _lib.u64p),
                                             _ptr(flipped, _lib.u8p), _ptr(n_var, _lib.u32p), _ptr(bad, _lib.u8p), _ptr(recs, _lib.i32p), _ptr(snip_ptr, _lib.u64p),
                                             _ptr(snip_c, _lib.u8p), _ptr(snip_t, _lib.u8p), cap, ctypes.byref(needed), ctypes.byref(ms))
        EDGE_VARIANT_STATS["kernel_ms"] += ms.value
        if rc == _lib.ISOCON_E_CAPACITY:
            cap = int(needed.value) + 64
            continue
        _lib.check(rc, "isocon_edge_variants")
        break
    EDGE_VARIANT_STATS["calls"] += 1          # (a call repeated with larger snippet buffers counts once)
    EDGE_VARIANT_STATS["edges"] += n
    total = int(snip_ptr[n_slots])
    return (flipped[:n], n_var[:n], bad[:n], recs[:n_slots], snip_ptr.astype(np.int64), snip_c[:total].tobytes().decode("ascii"), snip_t[:total].tobytes().decode("ascii"),
            rec_ptr.astype(np.int64))


def _tuples_from_edge_records(n, n_var, recs, snip_ptr, snip_c, snip_t, rec_ptr):
    """the _EdgeVariants of _edge_variants for every edge of an isocon_edge_variants answer"""
    R = recs.tolist()
    sp = snip_ptr.tolist()
    first = (rec_ptr - rec_ptr[0]).tolist() if n else [0]
    counts = n_var.tolist()
    out = []
    for e in range(n):
        rows = []
        for s in range(first[e], first[e] + counts[e]):
            i, _, _, key_t, key_c, u_v, _, packed = R[s]
            rows.append((i, key_t, key_c, u_v, chr(packed & 255), chr(packed >> 8 & 255), chr(packed >> 16 & 255), snip_c[sp[s]:sp[s + 1]], snip_t[sp[s]:sp[s + 1]]))
        out.append(_file_variant_records(rows))
    return out


def _edge_variants_on_device(live, C, ops, ops_ptr):
    """[_edge_variants(t, c, alignment (t, c), alignment (c, t))] for the edges (c_acc, t_acc) of `live` from the alignments' ops -- list 2 k
    = ops[ops_ptr[2 k]:ops_ptr[2 k + 1]] the (t, c) alignment of edge k, list 2 k + 1 the (c, t) one -- without the gapped strings:
    isocon_edge_variants, one call per EDGE_VARIANT_BATCH edges.  Equal under == and in the dicts' key order."""
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    ops_ptr = np.asarray(ops_ptr, dtype=np.int64)
    out = []
    for lo in range(0, len(live), EDGE_VARIANT_BATCH):
        part = live[lo:lo + EDGE_VARIANT_BATCH]
        index, seqs = {}, []
        for e in part:
            for acc in e:
                if acc not in index:
                    index[acc] = len(seqs)
                    seqs.append(C[acc])
        edge_c = [index[c_acc] for c_acc, _ in part]
        edge_t = [index[t_acc] for _, t_acc in part]
        ptr = ops_ptr[2 * lo:2 * (lo + len(part)) + 1]
        flipped, n_var, bad, recs, snip_ptr, snip_c, snip_t, rec_ptr = _edge_variants_call(seqs, edge_t, edge_c, ops[int(ptr[0]):int(ptr[-1])], ptr - ptr[0])
        if bad.any():
            raise RuntimeError("isocon_edge_variants: the ops of edge %r do not spell its two sequences" % (part[int(np.flatnonzero(bad)[0])],))
        out.extend(_tuples_from_edge_records(len(part), n_var, recs, snip_ptr, snip_c, snip_t, rec_ptr))
    return out


def _edge_variants(t_seq, c_seq, alignment_tc, alignment_ct):
    """_EdgeVariants (variants, variant_coords_t, variant_coords_c, alignment_c_to_t, alignment_t_to_c) of an edge from its two alignments"""
    aln_t, aln_c, variants = _candidate_vs_reference(alignment_tc, alignment_ct)
    return _EdgeVariants(variants, *functions.get_variant_coordinates(t_seq, c_seq, aln_t, aln_c, variants))


def _test_on_tables(t_seq, c_seq, alignment_tc, alignment_ct, tab_c, tab_t, ccs_dict=None, max_phred_q_trusted=None):
    """_test_on_alignments on the read tables of c and t: same tuple, the supporting reads as a count."""
    ev = _edge_variants(t_seq, c_seq, alignment_tc, alignment_ct)
    work_c = _SideWork(tab_c, np.flatnonzero(tab_c.agree_with_candidate(ev.coords_c)))
    work_t = _SideWork(tab_t, np.flatnonzero(tab_t.show_snippets(ev.coords_t, ev.c_to_t)))
    return _test_on_supporters(t_seq, ev, work_c, work_t, ccs_dict, max_phred_q_trusted)


def _test_on_supporters(t_seq, ev, work_c, work_t, ccs_dict=None, max_phred_q_trusted=None, pending=None):
    """The test of the edge ev (_EdgeVariants) once the supporting reads are known: error probabilities per read and the bound.  work_c / work_t
    (_SideWork): the tables of c / t, host or device alike, their supporting rows and a device table's answer about qualities.  pending: the round's collector."""
    variant_coords_t, tab_c, tab_t, sup_c, sup_t = ev.coords_t, work_c.tab, work_t.tab, work_c.supporters, work_t.supporters
    n_support = len(sup_c) + len(sup_t)
    if len(ev.variants) == 0:
        return variant_coords_t, 0.0, n_support, tab_c.n + tab_t.n
    if ccs_dict:
        # base qualities (functions.get_read_ccs_probabilities_c / _t): c's informative reads first, then t's
        ratios = None if work_c.probs is not None and work_t.probs is not None else _error_ratios(tab_c, tab_t)          # (the device had them with its queries)
        alive_c, prob_c = _ccs_probabilities_on_table(_SIDE_C, work_c, ev, ccs_dict, ratios, max_phred_q_trusted)
        alive_t, prob_t = _ccs_probabilities_on_table(_SIDE_T, work_t, ev, ccs_dict, ratios, max_phred_q_trusted)
        prob = np.concatenate([prob_c[alive_c], prob_t[alive_t]])
        if len(prob) == 0:
            assert n_support == 0
            return variant_coords_t, 0.0, n_support, 0
        assert alive_c[sup_c].all() and alive_t[sup_t].all()
        slot_c = np.cumsum(alive_c) - 1                       # position of a read of c among the informative ones
        slot_t = int(alive_c.sum()) + np.cumsum(alive_t) - 1
        return variant_coords_t, _raghavan_on_arrays(prob, np.concatenate([slot_c[sup_c], slot_t[sup_t]]) if n_support else None, pending), n_support, len(prob)
    # error probabilities per read, t's reads first (functions.get_read_errors / get_empirical_error_probabilities)
    n_reads = tab_t.n + tab_c.n
    if n_reads == 0:
        assert n_support == 0
        return variant_coords_t, 0.0, n_support, 0
    delta_size = float(len(variant_coords_t))
    seg = float(len(t_seq))
    p_S = (np.maximum(np.concatenate([tab_t.sub, tab_c.sub]), delta_size) / seg) / 3.0
    p_I = (np.maximum(np.concatenate([tab_t.ins, tab_c.ins]), delta_size) / seg) / 4.0
    p_D = np.maximum(np.concatenate([tab_t.dele, tab_c.dele]), delta_size) / seg
    prob = np.ones(n_reads, dtype=np.float64)
    for v_type, _, u_v in variant_coords_t.values():
        if v_type == "S":
            prob *= p_S * u_v
        elif v_type == "I":
            prob *= np.minimum(0.5, p_I * u_v)
        elif v_type == "D":
            prob *= np.minimum(0.5, p_D * u_v)
    prob[prob >= 1.0] = 0.99999
    return variant_coords_t, _raghavan_on_arrays(prob, np.concatenate([tab_t.n + sup_c, sup_t]) if n_support else None, pending), n_support, n_reads


def _raghavan_on_arrays(prob, supporters, pending=None):
    """raghavan_upper_pvalue_bound for probabilities in dict order and the indices of the supporting reads (in the order of
    functions.get_support): logarithms with math.log per distinct probability, sums left to right like the reference's.  pending: a list
    that takes (m_sum, y_sum) in place of the evaluation -- a _PendingBound comes back, for _resolve_bounds."""
    assert prob.max() <= 1.0 and prob.min() > 0.0
    uniq, inv = np.unique(prob, return_inverse=True)
    logs = [-math.log(p, 10) for p in uniq.tolist()]
    log_max = max(logs)
    assert log_max > 0
    w_u = np.asarray([l / log_max for l in logs], dtype=np.float64)
    weight = w_u[inv]
    m_sum = sum((w_u * uniq)[inv].tolist())
    y_sum = sum(weight[supporters].tolist()) if supporters is not None else 0
    if pending is not None:
        pending.append((m_sum, y_sum))
        return _PendingBound(len(pending) - 1)
    return _raghavan_from_sums(m_sum, y_sum)


def arrange_alignments_new_no_realign(t_acc, c_acc, t_seq, c_seq, read_alignments_to_c, read_alignments_to_t, ccs_dict, ignore_ends_len, max_phred_q_trusted):
    """hypothesis_test_module.py:92-171 (single edge; the batch entry point is do_statistical_tests_per_edge)."""
    tc, ct = SWM._align_pairs([(t_seq, c_seq), (c_seq, t_seq)], [-3, -3], 2, 3, 1)
    return _test_on_alignments(t_seq, c_seq, tc, ct, read_alignments_to_c, read_alignments_to_t, ccs_dict, max_phred_q_trusted)


def _result(c_acc, t_acc, t_seq, variant_coords_t, p_value, reads_support, nr_reads_used, with_qualities=False):
    variant_types = ";".join("(" + str(v[0]) + "," + str(j) + "," + str(v[2]) + ")" for j, v in variant_coords_t.items())
    factor = 1.0 if with_qualities else get_correction_factor(t_seq, c_acc, variant_coords_t)      # :242-246
    return (c_acc, t_acc, p_value, factor, len(reads_support), nr_reads_used, variant_types)


def statistical_test(c_acc, t_acc, c_seq, t_seq, reads_to_c, read_alignments_to_t, read_alignments_to_c, ignore_ends_len, ccs_dict, max_phred_q_trusted):
    """hypothesis_test_module.py:217-247: (c_acc, t_acc, p_value, correction factor, supporting reads, reads used, variants)."""
    assert not (set(reads_to_c) & set(read_alignments_to_t))
    N_t = len(set(reads_to_c) | set(read_alignments_to_t))
    if N_t == 0:    # all reads of both went elsewhere in the realignment
        return c_acc, t_acc, 1.0, 1.0, 0, N_t, ""
    if ccs_dict:
        for x_acc in reads_to_c:
            assert reads_to_c[x_acc] == ccs_dict[x_acc].seq
    delta_t, p_value, reads_support, used = arrange_alignments_new_no_realign(t_acc, c_acc, t_seq, c_seq, read_alignments_to_c, read_alignments_to_t,
                                                                              ccs_dict, ignore_ends_len, max_phred_q_trusted)
    return _result(c_acc, t_acc, t_seq, delta_t, p_value, reads_support, used, bool(ccs_dict))


def _tests_of(live, C, read_partition, ccs_dict, params, routes, at=None):
    """The tests of the edges `live` (each with reads on c or on t), in that order: the alignments of their candidates in one batch, their
    variants in one device call, the tests on the device tables -- or, where routes says so, on the host tables.  Returns (of_edge, test):
    `e in of_edge` iff e is one of `live`; test(e) = (variant_coords_t, p_value, supporting reads, reads used), already there on the device
    route, evaluated when asked on the host tables.  at: see _tests_on_device."""
    max_q = getattr(params, "max_phred_q_trusted", None)
    pairs = [pair for c, t in live for pair in ((C[t], C[c]), (C[c], C[t]))]
    if pairs and routes.variants:
        # the alignments stay ops: variants, coordinates and snippets of all edges from the device, gapped strings only on demand
        ops, ops_ptr = SWM._align_pairs(pairs, [-3] * len(pairs), 2, 3, 1, want_ops=True)
        of_edge = _LazyAlignments(live, C, ops, ops_ptr)
        variants_of = dict(zip(live, _edge_variants_on_device(live, C, ops, ops_ptr)))
    else:
        alignments = SWM._align_pairs(pairs, [-3] * len(pairs), 2, 3, 1) if pairs else []
        of_edge = {e: (alignments[2 * i], alignments[2 * i + 1]) for i, e in enumerate(live)}
        variants_of = None
    if routes.tables:
        return of_edge, _tests_on_device(live, of_edge, C, read_partition, ccs_dict, max_q, variants_of, routes, at).__getitem__
    tables = _tables_for([(C[acc], read_partition[acc]) for e in live for acc in e])

    def on_host_tables(e):
        tc, ct = of_edge[e]
        return _test_on_tables(C[e[1]], C[e[0]], tc, ct, tables[id(read_partition[e[0]])], tables[id(read_partition[e[1]])], ccs_dict, max_q)

    return of_edge, on_host_tables


# ---- one process per GPU: a round's edges shared between the ranks (dist.shard_edges) ----
# rounds: the sharded rounds of this process; edges_owned / edges_total: the live edges this rank tested itself / all live edges of those
# rounds; gather_bytes: the pickled rows (and exception) this rank put into the rounds' all_gather_object
SHARD_STATS = {"rounds": 0, "edges_owned": 0, "edges_total": 0, "gather_bytes": 0}


def _sharing_group():
    """torch.distributed when a round's edges are shared between the ranks: the caller runs one process per GPU (world size above 1) and
    ISOCON_DEBUG_VARIANT=stat_all_edges -- every rank tests all edges itself -- is not set"""
    from .nearest_neighbor_graph import _process_group
    listed = {item.split("=")[0] for item in os.environ.get("ISOCON_DEBUG_VARIANT", "").split(",")}
    return None if "stat_all_edges" in listed else _process_group()


def _travels(exc):
    """exc if it survives pickling (all_gather_object), else a RuntimeError that quotes it"""
    import pickle
    try:
        pickle.loads(pickle.dumps(exc))
        return exc
    except Exception:          # noqa: BLE001
        return RuntimeError("do_statistical_tests_per_edge: %r" % (exc,))


def _shared_rows(group, edges, live, C, read_partition, ccs_dict, params, routes):
    """{edge: _result(...)[2:]} for all edges of `live`, each tested by ONE rank of the group: the edges are dealt by dist.shard_edges (weight 1
    + the reads of c and of t), a rank runs _tests_of and _result for its own edges in its own order, one all_gather_object brings every rank's
    rows (doubles travel exactly) to every rank.  Collectives per round: one reduction that confirms that the ranks hold the same edges and
    weights (a RuntimeError on every rank otherwise), and the gather.  A rank whose share raises -- SystemExit and AssertionError are among
    what a test raises -- stops there, sends the exception with its edge in place of the remaining rows, and every rank raises, of the gathered
    exceptions, the one whose edge comes first in `edges`, its own order.  (With ONE raising edge that is what a single process raises.  With
    several it need not be: a single process goes through its edges in phases -- all tests on the device tables before the edges left to the
    host tables --, so there an edge whose device answer raises comes before an earlier edge that raises on the host tables.)"""
    import pickle
    from . import dist as D
    weights = [1 + len(read_partition[c]) + len(read_partition[t]) for c, t in live]
    if not D.same_everywhere(D.edge_digest(live, weights), group):
        raise RuntimeError("do_statistical_tests_per_edge: the ranks hold different edges / read partitions (digest mismatch); "
                           "every rank must run the same round on the same input")
    world, rank = group.get_world_size(), group.get_rank()
    mine = set(D.shard_edges(live, weights, world)[rank])
    own = [e for e in live if e in mine]
    rows, failed, at = {}, None, [None]
    try:
        if own:          # (a rank without an edge makes no device call)
            _, test = _tests_of(own, C, read_partition, ccs_dict, params, routes, at)
            for e in own:
                at[0] = e
                delta_t, p_value, n_support, used = test(e)
                rows[e] = _result(e[0], e[1], C[e[1]], delta_t, p_value, range(n_support), used, bool(ccs_dict))[2:]
    except (Exception, SystemExit) as exc:          # (what the tests themselves raise, not an interrupt); a failure of a whole batch counts for its first edge
        failed = (own[0] if at[0] is None else at[0], _travels(exc))
    SHARD_STATS["rounds"] += 1
    SHARD_STATS["edges_owned"] += len(own)
    SHARD_STATS["edges_total"] += len(live)
    sent = pickle.dumps((rows, failed), pickle.HIGHEST_PROTOCOL)          # pickled HERE, once: the gather then only copies the bytes, and their number is known
    SHARD_STATS["gather_bytes"] += len(sent)
    gathered = [None] * world
    group.all_gather_object(gathered, sent)
    gathered = [pickle.loads(part) for part in gathered]
    failures = [f for _, f in gathered if f is not None]
    if failures:
        place = {e: k for k, e in enumerate(edges)}
        raise min(failures, key=lambda f: place[f[0]])[1]
    return {e: row for part, _ in gathered for e, row in part.items()}


def do_statistical_tests_per_edge(nearest_neighbor_graph, C, X, read_partition, ccs_dict, params):
    """hypothesis_test_module.py:20-77: {c_acc: {t_acc: (p_value, correction factor, support, reads used, variants)}} for
    every edge c -> t of the graph (nr_cores is irrelevant here: one device batch for all edges; one process per GPU: one batch
    per rank for its share of the edges, _shared_rows)."""
    edges = [(c_acc, t_acc) for c_acc in nearest_neighbor_graph for t_acc in nearest_neighbor_graph[c_acc]]
    live = [(c, t) for c, t in edges if len(read_partition[c]) + len(read_partition[t]) > 0]
    p_values = {c_acc: {} for c_acc in nearest_neighbor_graph}
    routes = _routes()
    group = _sharing_group()
    if group is None:
        of_edge, test = _tests_of(live, C, read_partition, ccs_dict, params, routes)
    else:
        of_edge = _shared_rows(group, edges, live, C, read_partition, ccs_dict, params, routes)
    for c_acc, t_acc in edges:
        if (c_acc, t_acc) not in of_edge:
            p_values[c_acc][t_acc] = (1.0, 1.0, 0, 0, "")
            continue
        assert not (set(read_partition[c_acc]) & set(read_partition[t_acc]))
        if ccs_dict:
            for x_acc in read_partition[c_acc]:
                assert X[x_acc] == ccs_dict[x_acc].seq
        if group is None:
            delta_t, p_value, n_support, used = test((c_acc, t_acc))
            p_values[c_acc][t_acc] = _result(c_acc, t_acc, C[t_acc], delta_t, p_value, range(n_support), used, bool(ccs_dict))[2:]
        else:
            p_values[c_acc][t_acc] = of_edge[(c_acc, t_acc)]
    return p_values


def raghavan_upper_pvalue_bound(probability, x_equal_to_one):
    """hypothesis_test_module.py:253-329: Raghavan's bound for a weighted sum of independent Bernoulli variables,
    P(Y > m (1 + d)) < (e^d / (1 + d)^(1 + d))^m, with weights w_i = log10(p_i) / min log10(p) in (0, 1], Y = the summed
    weights of the supporting reads, m = E[Y]; evaluated as e^k / (1 + d)^(k + k / d), k = m d, in 100-digit decimals
    (the reference sets that precision module-wide)."""
    assert max(probability.values()) <= 1.0
    assert min(probability.values()) > 0.0
    log_probabilities = {acc: -math.log(p_i, 10) for acc, p_i in probability.items()}
    log_p_i_max = max(log_probabilities.values())
    assert log_p_i_max > 0
    weight = {acc: log_probabilities[acc] / log_p_i_max for acc in log_probabilities}
    return _raghavan_from_sums(sum([weight[acc] * probability[acc] for acc in probability]), sum([weight[x_i] for x_i in x_equal_to_one]))


def _raghavan_from_sums(m_sum, y_sum):
    with decimal.localcontext() as ctx:
        ctx.prec = 100
        m = decimal.Decimal(m_sum)
        y = decimal.Decimal(y_sum)
        d = y / m - 1
        k = m * d
        if y == 0:
            bound = 1.0
        elif d == 0:
            bound = 0.5
        else:
            bound = k.exp() / (d + 1) ** (k + k / d)
        return float(bound)


def get_correction_factor(t_seq, c_acc, delta_t):
    """hypothesis_test_module.py:331-343: the number of candidates with the same numbers of substitutions, deletions and
    insertions relative to t (multiple-testing factor)."""
    m = len(t_seq)
    n_S = sum(1 for v in delta_t.values() if v[0] == "S")
    n_D = sum(1 for v in delta_t.values() if v[0] == "D")
    n_I = sum(1 for v in delta_t.values() if v[0] == "I")
    return ((4 * (m + 1)) ** n_I) * functions.choose(m, n_D) * functions.choose(3 * (m - n_D), n_S)
