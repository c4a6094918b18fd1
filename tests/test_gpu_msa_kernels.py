"""The consensus-correction kernels (csrc/msa.hpp) and their entry points (msa_host.inc) against the numpy
checker (oracle/correction.py) and the host matrix (functions.msa_matrix), on the designed inputs of tests/msa_cases.py: column ties,
gap majorities, zero class totals, frequency ties, the limits of the LDS candidate lists (2048; 1024 in the batched kernel, with the
single-partition repeat of correction_module), centres at the 1024-slot step of the layout scan, rows with more than 64 ops, insertions
around the 32 coded bases of a wide record, and every refusal of the entry points.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import msa_cases as MC
from oracle import correction as OC

pytestmark = pytest.mark.gpu

GAP = 45
OK, E_ARG, E_ALPHABET, E_CAPACITY = 0, -1, -2, -4
SENTINEL = 0xA5A5A5A5


def _p(a, t):
    return a.ctypes.data_as(t)


def _rows(packed, off):
    return [bytes(packed[int(off[r]):int(off[r + 1])]) for r in range(len(off) - 1)]


# ---- 1. isocon_msa_correct on designed matrices -----------------------------------------------------------------------------------------

def correct_abi(M, deg, packed_cap=None):
    """isocon_msa_correct with its class totals -> (rc, packed, offsets, n_cand, (c_ins, c_del, c_subs))"""
    from isocon_amd import _lib
    L = _lib.lib()
    M = np.ascontiguousarray(M, dtype=np.uint8)
    nr, ncols = M.shape
    deg32 = np.ascontiguousarray(deg, dtype=np.int32)
    cap = M.size if packed_cap is None else packed_cap
    packed = np.full(max(cap, 1), 0, dtype=np.uint8)
    off = np.zeros(nr + 1, dtype=np.uint64)
    n_cand = np.full(nr, -7, dtype=np.int32)
    tot = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = L.isocon_msa_correct(_p(M, _lib.u8p), nr, ncols, _p(deg32, _lib.i32p), _p(packed, _lib.u8p), cap, _p(off, _lib.u64p), _p(n_cand, _lib.i32p), tot, None)
    return rc, packed, off.astype(np.int64), n_cand, tuple(int(x) for x in tot)


def assert_equals_checker(M, deg):
    rc, packed, off, n_cand, tot = correct_abi(M, deg)
    assert rc == OK
    p2, o2, n2 = OC.correct_rows(M, deg)
    assert n_cand.tolist() == n2.tolist()
    assert off.tolist() == o2.tolist()
    assert bytes(packed[:off[-1]]) == p2.tobytes()
    assert tot == OC.class_totals(M, deg)
    return packed, off, n_cand, tot


CASES = {name: (M, deg) for name, M, deg in MC.correct_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_correct_equals_checker(name):
    M, deg = CASES[name]
    packed, off, n_cand, tot = assert_equals_checker(M, deg)
    # the branch the case was built for was reached
    if name.startswith("a_"):
        assert (n_cand == 0).all() and tot == (0, 0, 0)
    if name.startswith("c_all_rows_empty"):
        assert n_cand.sum() > 0 and (off == 0).all()
    if name.startswith("c_empty_middle"):
        assert off[1] == off[2] and n_cand[1] == M.shape[1]
    if name.startswith("d_only_substitutions"):
        assert tot[0] == 0 and tot[1] == 0 and tot[2] > 0 and n_cand.min() > 0
    if name.startswith("d_only_insertions"):
        assert tot[1] == 0 and tot[2] == 0 and tot[0] > 0
    if name.startswith("e_"):
        assert (n_cand[np.asarray(deg) != 1] == 0).all() and sorted(np.asarray(deg)[np.asarray(deg) != 1].tolist()) == [2, 3, 50]
    if name.startswith("g_list_limit"):
        n = int(name.rsplit("_", 1)[1])
        assert n_cand[4] == n and n_cand[:3].tolist() == [0, 0, 0]          # 2047 / 2048: the list in LDS, its last entry; 2049: the repeat launch


@pytest.mark.parametrize("nr,ncols,seed", [(5, 65, 23), (9, 255, 24)])
def test_tied_columns_are_never_corrected(nr, ncols, seed):
    """(b) a column whose maximum is shared -- by two to five symbols, '-' among them -- keeps every row's symbol"""
    M, deg, ties = MC.subset_ties(nr, ncols, seed)
    packed, off, n_cand, tot = assert_equals_checker(M, deg)
    # with every OTHER column made unanimous, nothing is a candidate: the tie flag alone decides
    only = np.tile(M[0], (nr, 1))
    cols = [c for c, _ in ties]
    only[:, cols] = M[:, cols]
    packed, off, n_cand, tot = assert_equals_checker(only, deg)
    assert (n_cand == 0).all() and tot == (0, 0, 0)
    assert _rows(packed, off) == [only[r][only[r] != GAP].tobytes() for r in range(nr)]


@pytest.mark.parametrize("name", sorted(MC.TIE_SPECS))
def test_frequency_ties_against_rational_arithmetic(name):
    """(f) equal rationals from different integers (4/12, 6/18, 7/21), the ceil(n / 2)-th smallest inside, first and last of a tie group,
    n = 1, 2, odd, even: the target row equals what exact fractions give"""
    M, deg, want_row, n_corrected = MC.freq_ties(MC.TIE_SPECS[name], 300, 256, 50)
    packed, off, n_cand, tot = assert_equals_checker(M, deg)
    assert tot == MC.TIE_TOTALS and n_cand[MC.TIE_ROW] == len(MC.TIE_SPECS[name])
    assert _rows(packed, off)[MC.TIE_ROW] == want_row.tobytes()


# ---- 2. the matrix from ops, one partition and batched ------------------------------------------------------------------------------------

class World(object):
    """the partitions of a list in one store, with the single-partition device results kept for the batched comparison"""

    def __init__(self, parts):
        from isocon_amd.store import SeqStore
        self.C = MC.Concatenation(parts)
        self.store = SeqStore(list(self.C.seqs))
        self.single = {}

    def patches(self, i, wide, col_slot, longest):
        from isocon_amd import correction_module as COR
        return COR._wide_slot_patches(self.C.parts[i].members, wide, col_slot, longest)

    def build_single(self, i):
        """-> (n_cols, col_slot, longest, wide, patches, matrix with the patches applied)"""
        rows, ops, ptr = self.C.single(i)
        n_cols, col_slot, longest, wide = self.store.msa_build_ops(rows, ops, ptr)
        dev = self.store.msa_read_built(len(rows), n_cols)
        pt = self.patches(i, wide, col_slot, longest)
        for k in range(0 if pt[0] is None else len(pt[0])):
            dev[pt[0][k], pt[1][k]:pt[1][k] + int(pt[2][k + 1] - pt[2][k])] = pt[3][int(pt[2][k]):int(pt[2][k + 1])]
        return n_cols, col_slot, longest, wide.copy(), pt, dev


def sorted_records(wide):
    return sorted(map(tuple, np.asarray(wide, dtype=np.int64).tolist()))


@pytest.fixture(scope="module")
def world():
    P = MC.build_partitions()
    w = World([P[k] for k in MC.BATCH_ORDER])
    yield w
    w.store.close()


@pytest.mark.parametrize("i", range(len(MC.BATCH_ORDER)), ids=MC.BATCH_ORDER)
def test_built_matrix_equals_host_matrix(world, i):
    p = world.C.parts[i]
    host, longest_h, col_slot_h = p.host()
    n_cols, col_slot, longest, wide, pt, dev = world.build_single(i)
    assert n_cols == host.shape[1]
    assert col_slot.tolist() == col_slot_h.tolist() and longest.tolist() == longest_h.tolist()
    assert dev.shape == host.shape and (dev == host).all()
    # one record per insertion into a wide slot: row, slot, position in the member, length, the first 32 bases
    want = []
    for r, t, s in p.insertions():
        if longest_h[t] > 1:
            a1, a2 = p.pairs[r - 1]
            sp = len(a2[:_column_of_slot(a1, t)].replace("-", ""))
            codes = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(s[:32]))
            want.append((r, t, sp, len(s), codes & 0xffffffff, codes >> 32, 0, 0))
    assert sorted_records(wide) == sorted(want)
    # the correction on the built matrix
    packed, off, n_cand = world.store.msa_correct_built(p.n_rows, n_cols, p.deg, *pt)
    p2, o2, n2 = OC.correct_rows(host, p.deg)
    assert n_cand.tolist() == n2.tolist() and off.tolist() == o2.tolist() and bytes(packed[:off[-1]]) == p2.tobytes()
    world.single[i] = (wide, _rows(packed, off), n_cand.tolist())


def _column_of_slot(a1, t):
    """index in the gapped centre where slot t starts (t centre bases in front of it)"""
    seen = 0
    for i, ch in enumerate(a1):
        if seen == t:
            return i
        seen += ch != "-"
    return len(a1)


def batch_patches(world, first_row, slot_base, col_slot, longest, wide):
    """the patches of a batch: _wide_slot_patches per partition on its own records, rows shifted back to the concatenation"""
    rows_l, cols_l, lens_l, bytes_l = [], [], [], []
    for i in sorted(set(wide[:, 6].tolist())):
        local = wide[wide[:, 6] == i].copy()
        r0, sb, se = int(first_row[i]), int(slot_base[i]), int(slot_base[i + 1])
        local[:, 0] -= r0
        pr, pc, pp, pb = world.patches(i, local, col_slot[sb:se], longest[sb:se])
        rows_l.append(np.asarray(pr, dtype=np.int64) + r0)
        cols_l.append(np.asarray(pc, dtype=np.int64))
        lens_l.append(np.diff(pp.astype(np.int64)))
        bytes_l.append(pb)
    if not rows_l:
        return None, None, None, None
    p_ptr = np.zeros(sum(len(x) for x in rows_l) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(lens_l), out=p_ptr[1:])
    return np.concatenate(rows_l), np.concatenate(cols_l), p_ptr, np.concatenate(bytes_l)


def run_batch(world):
    C = world.C
    n_cols, slot_base, col_slot, longest, wide = world.store.msa_build_ops_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)
    wide = wide.copy()
    pt = batch_patches(world, C.first_row, slot_base, col_slot, longest, wide)
    cap = int(sum(len(s) for s in C.seqs)) + 16 * C.n_rows + 1024
    packed, off, n_cand = world.store.msa_correct_built_batch(len(C.parts), C.n_rows, C.deg, cap, *pt)
    return n_cols, slot_base, col_slot, longest, wide, _rows(packed, off), n_cand


def test_batched_build_and_correct_equal_host_and_single(world):
    C = world.C
    for i in range(len(C.parts)):
        if i not in world.single:
            test_built_matrix_equals_host_matrix(world, i)
    n_cols, slot_base, col_slot, longest, wide, rows, n_cand = run_batch(world)
    assert len(wide) > 100 and set(wide[:, 6].tolist()) == set(range(len(C.parts)))          # every partition has wide slots
    for i, p in enumerate(C.parts):
        host, longest_h, col_slot_h = p.host()
        r0, r1, sb, se = int(C.first_row[i]), int(C.first_row[i + 1]), int(slot_base[i]), int(slot_base[i + 1])
        assert n_cols[i] == host.shape[1] and se - sb == len(p.centre) + 1
        assert col_slot[sb:se].tolist() == col_slot_h.tolist() and longest[sb:se].tolist() == longest_h.tolist()
        # the records: word 6 the partition, word 0 the row of the concatenation; as a set, the single-partition records shifted
        mine = wide[wide[:, 6] == i]
        assert ((mine[:, 0] >= r0) & (mine[:, 0] < r1)).all()
        shifted = mine.astype(np.int64)
        shifted[:, 0] -= r0
        shifted[:, 6] = 0
        wide_1, rows_1, n_cand_1 = world.single[i]
        assert sorted_records(shifted) == sorted_records(wide_1)
        # the corrected rows: the checker on the HOST matrix, and the single-partition device calls
        p2, o2, n2 = OC.correct_rows(host, p.deg)
        assert n_cand[r0:r1].tolist() == n2.tolist()
        assert rows[r0:r1] == _rows(p2, o2)
        assert rows[r0:r1] == rows_1 and n_cand[r0:r1].tolist() == n_cand_1


# ---- 3. the batched kernel's list limit and the repeat through the single-partition path ---------------------------------------------------

@pytest.fixture(scope="module")
def limit_world():
    w = World(MC.limit_partitions())
    yield w
    w.store.close()


def test_batched_list_limit_through_the_abi(limit_world):
    C = limit_world.C
    names = [p.name for p in C.parts]
    n_cols, slot_base, col_slot, longest, wide, rows, n_cand = run_batch(limit_world)
    over = int(C.first_row[names.index("limit1025")]) + 1
    assert np.flatnonzero(n_cand < 0).tolist() == [over] and n_cand[over] == -1
    at_limit = int(C.first_row[names.index("limit1024")]) + 1
    assert n_cand[at_limit] == 1024          # the last entry of the LDS list
    for i, p in enumerate(C.parts):
        r0, r1 = int(C.first_row[i]), int(C.first_row[i + 1])
        p2, o2, n2 = OC.correct_rows(p.host()[0], p.deg)
        if p.name == "limit1025":
            assert n2[1] == 1025
            keep = [r for r in range(p.n_rows) if r != 1]          # the other rows of that partition are not touched by the overflow
            assert [n_cand[r0 + r] for r in keep] == [n2[r] for r in keep]
            assert [rows[r0 + r] for r in keep] == [_rows(p2, o2)[r] for r in keep]
        else:
            assert n_cand[r0:r1].tolist() == n2.tolist() and rows[r0:r1] == _rows(p2, o2)
    # the single-partition kernels take the 1025 row (their list holds 2048)
    i = names.index("limit1025")
    p = C.parts[i]
    n_cols_1, col_slot_1, longest_1, wide_1, pt, dev = limit_world.build_single(i)
    assert (dev == p.host()[0]).all()
    packed, off, n1 = limit_world.store.msa_correct_built(p.n_rows, n_cols_1, p.deg, *pt)
    p2, o2, n2 = OC.correct_rows(p.host()[0], p.deg)
    assert n1.tolist() == n2.tolist() and n1[1] == 1025 and _rows(packed, off) == _rows(p2, o2)


def designed_partition_alignments(parts, store):
    """what isocon_get_candidates.get_partition_alignments returns for these partitions, made from their scripted alignments: a
    PartitionAlignments with a live AlignmentBatch over `store` (which holds the partitions' sequences in order) -> (pa, seq_to_acc, seqs)"""
    from isocon_amd import isocon_get_candidates as IGC
    seqs = [s for p in parts for s in p.seqs]
    pairs, a, b, ops, edit = [], [], [], [], []
    first = 0
    for p in parts:
        for j, m in enumerate(p.members):
            pairs.append((p.centre, m))
            a.append(first)
            b.append(first + 1 + j)
            ops.append(p.ops[j])
            edit.append(int(sum(int(o) >> 4 for o in p.ops[j] if int(o) & 15)))
        first += p.n_rows
    ops_ptr = np.zeros(len(pairs) + 1, dtype=np.int64)
    np.cumsum([len(o) for o in ops], out=ops_ptr[1:])
    batch = IGC.AlignmentBatch(store, pairs, np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32), np.concatenate(ops).astype(np.uint32), ops_ptr, None)
    pa = IGC.PartitionAlignments()
    pa.batch = batch
    k = 0
    for p in parts:
        pa[p.centre] = {p.centre: (0, p.centre, p.centre, int(p.degree))}
        for m in p.members:
            pa[p.centre][m] = IGC.LazyAlignment(batch, k, edit[k])
            batch.rows_of.setdefault(p.centre, []).append(k)
            k += 1
    return pa, {s: ["read%d" % i] for i, s in enumerate(seqs)}, seqs


def test_correct_strings_repeats_the_overflowing_partition(monkeypatch):
    """correction_module.correct_strings on a PartitionAlignments with a live batch: the partition whose row overflows the batched list is
    corrected again through _correct_partition_from_ops, the rows the batched call returned for it are dropped, nothing is lost or doubled"""
    from isocon_amd import correction_module as COR
    from isocon_amd.store import SeqStore
    parts = MC.limit_partitions()
    store = SeqStore([s for p in parts for s in p.seqs])
    try:
        pa, seq_to_acc, seqs = designed_partition_alignments(parts, store)
        calls, batched_part = [], []
        inner_single, inner_all = COR._correct_partition_from_ops, COR._correct_all_from_ops

        def counting_single(batch_, m, partition, acc):
            out = inner_single(batch_, m, partition, acc)
            calls.append((m, sorted(out)))
            return out

        def recording_all(*args):
            part, redo = inner_all(*args)
            batched_part.append((sorted(part), list(redo)))
            return part, redo

        monkeypatch.setattr(COR, "_correct_partition_from_ops", counting_single)
        monkeypatch.setattr(COR, "_correct_all_from_ops", recording_all)
        dev, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
        over = [p for p in parts if p.name == "limit1025"][0]
        assert len(batched_part) == 1 and batched_part[0][1] == [over.centre]          # the redo list: that partition, once
        assert [m for m, _ in calls] == [over.centre]
        redone = calls[0][1]
        assert "read%d" % seqs.index(over.members[0]) in redone
        assert not set(redone) & set(batched_part[0][0])                              # no accession from both sources
        assert sorted(dev) == sorted(redone + batched_part[0][0])
        # the string path with the numpy checker
        monkeypatch.setattr(COR, "_correct_on_device", OC.correct_rows)
        host, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
        assert len(calls) == 1                                                        # (the string path does not come here)
        assert dev == host
        n_corrected = sum(int(((OC.correct_rows(p.host()[0], p.deg)[2] > 0) & (p.deg == 1)).sum()) for p in parts)
        assert len(dev) == n_corrected and len(dev) > 20
    finally:
        store.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------

class Refusals(object):
    """a store with a good partition (rows 0 ..), a longer one with a many-op member, and two spare sequences; raw entry points"""

    def __init__(self):
        from isocon_amd import _lib
        from isocon_amd.store import SeqStore
        rng = np.random.default_rng(123)
        c = MC.random_seq(rng, 40)
        self.good = MC.Partition("good", c, [[("I", 5, "AC"), ("X", 9)], [("I", 5, "G"), ("D", 20, 2)], [("I", 0, "TTT"), ("I", 40, "GA")], [("X", 3)]], degree=2)
        c2 = MC.random_seq(rng, 200)
        self.many = MC.Partition("many", c2, [MC.n_ops_member(c2, 100), [("I", 150, "ACGT")], [("I", 150, "CC"), ("I", 199, "TT")]])
        self.C = MC.Concatenation([self.good, self.many])
        self.spare_longer = self.C.n_rows          # the centre of `good` plus one base
        self.seqs = list(self.C.seqs) + [c + "A"]
        self.store = SeqStore(list(self.seqs))
        self.L, self.lib = _lib.lib(), _lib
        self.h = self.store.handle

    def build(self, row_ids, ops, ops_ptr, wide_cap=64):
        lib = self.lib
        row_ids = np.ascontiguousarray(row_ids, dtype=np.uint32)
        ops = np.ascontiguousarray(ops if len(ops) else np.zeros(1), dtype=np.uint32)
        ops_ptr = np.ascontiguousarray(ops_ptr, dtype=np.uint64)
        n_slots = int(max(len(s) for s in self.seqs)) + 1
        n_cols, n_wide = ctypes.c_uint32(SENTINEL), ctypes.c_uint64(SENTINEL)
        col_slot, longest = np.zeros(n_slots, dtype=np.uint32), np.zeros(n_slots, dtype=np.uint32)
        wide = np.full((max(wide_cap, 1), 8), SENTINEL, dtype=np.uint32)
        rc = self.L.isocon_msa_build_ops(self.h, len(row_ids), _p(row_ids, lib.u32p), _p(ops, lib.u32p), _p(ops_ptr, lib.u64p), ctypes.byref(n_cols),
                                         _p(col_slot, lib.u32p), _p(longest, lib.u32p), _p(wide, lib.u32p), wide_cap, ctypes.byref(n_wide), None)
        return rc, int(n_cols.value), int(n_wide.value), wide

    def build_batch(self, first_row, row_ids, ops, ops_ptr, wide_cap=64):
        lib = self.lib
        first_row = np.ascontiguousarray(first_row, dtype=np.uint32)
        row_ids = np.ascontiguousarray(row_ids, dtype=np.uint32)
        ops = np.ascontiguousarray(ops if len(ops) else np.zeros(1), dtype=np.uint32)
        ops_ptr = np.ascontiguousarray(ops_ptr, dtype=np.uint64)
        n_parts = len(first_row) - 1
        n_slots = n_parts * (int(max(len(s) for s in self.seqs)) + 1)
        n_cols, n_wide = np.full(n_parts, SENTINEL, dtype=np.uint32), ctypes.c_uint64(SENTINEL)
        col_slot, longest = np.zeros(n_slots, dtype=np.uint32), np.zeros(n_slots, dtype=np.uint32)
        wide = np.full((max(wide_cap, 1), 8), SENTINEL, dtype=np.uint32)
        rc = self.L.isocon_msa_build_ops_batch(self.h, n_parts, _p(first_row, lib.u32p), _p(row_ids, lib.u32p), _p(ops, lib.u32p), _p(ops_ptr, lib.u64p),
                                               _p(n_cols, lib.u32p), _p(col_slot, lib.u32p), _p(longest, lib.u32p), _p(wide, lib.u32p), wide_cap, ctypes.byref(n_wide), None)
        return rc, n_cols, int(n_wide.value), wide

    def correct_built(self, n_rows, n_cols, deg, pt=(None, None, None, None), packed_cap=None):
        lib = self.lib
        deg = np.ascontiguousarray(deg, dtype=np.int32)
        n_p = 0 if pt[0] is None else len(pt[0])
        arrs = [np.ascontiguousarray(x if n_p else np.zeros(2), dtype=t) for x, t in zip(pt, (np.uint32, np.uint32, np.uint32, np.uint8))]
        cap = n_rows * n_cols if packed_cap is None else packed_cap
        packed = np.zeros(max(cap, 1), dtype=np.uint8)
        off = np.zeros(n_rows + 1, dtype=np.uint64)
        n_cand = np.zeros(n_rows, dtype=np.int32)
        rc = self.L.isocon_msa_correct_built(self.h, n_rows, n_cols, _p(arrs[0], lib.u32p), _p(arrs[1], lib.u32p), _p(arrs[2], lib.u32p), _p(arrs[3], lib.u8p), n_p,
                                             _p(deg, lib.i32p), _p(packed, lib.u8p), cap, _p(off, lib.u64p), _p(n_cand, lib.i32p), None, None)
        return rc, packed, off.astype(np.int64), n_cand

    def correct_built_batch(self, n_parts, n_rows, deg, pt, packed_cap):
        lib = self.lib
        deg = np.ascontiguousarray(deg, dtype=np.int32)
        n_p = 0 if pt[0] is None else len(pt[0])
        arrs = [np.ascontiguousarray(x if n_p else np.zeros(2), dtype=t) for x, t in zip(pt, (np.uint32, np.uint32, np.uint32, np.uint8))]
        packed = np.zeros(max(packed_cap, 1), dtype=np.uint8)
        off = np.zeros(n_rows + 1, dtype=np.uint64)
        n_cand = np.zeros(n_rows, dtype=np.int32)
        rc = self.L.isocon_msa_correct_built_batch(self.h, n_parts, n_rows, _p(arrs[0], lib.u32p), _p(arrs[1], lib.u32p), _p(arrs[2], lib.u32p), _p(arrs[3], lib.u8p), n_p,
                                                   _p(deg, lib.i32p), _p(packed, lib.u8p), packed_cap, _p(off, lib.u64p), _p(n_cand, lib.i32p), None)
        return rc, packed, off.astype(np.int64), n_cand

    def read_built(self, n_rows, n_cols):
        M = np.zeros((n_rows, max(n_cols, 1)), dtype=np.uint8)
        return self.L.isocon_msa_read_built(self.h, n_rows, n_cols, _p(M, self.lib.u8p)), M

    def still_works(self):
        """a correct build + correct of the good partition on the same store gives the right answer"""
        w = World.__new__(World)
        w.C, w.store, w.single = self.C, self.store, {}
        host = self.good.host()[0]
        n_cols, col_slot, longest, wide, pt, dev = w.build_single(0)
        assert (dev == host).all()
        packed, off, n_cand = self.store.msa_correct_built(self.good.n_rows, n_cols, self.good.deg, *pt)
        p2, o2, n2 = OC.correct_rows(host, self.good.deg)
        assert n_cand.tolist() == n2.tolist() and _rows(packed, off) == _rows(p2, o2)


@pytest.fixture(scope="module")
def ref():
    r = Refusals()
    yield r
    r.store.close()


def _op(n, code):
    return (n << 4) | "=XID".index(code)


def test_refused_ops_that_do_not_spell_the_sequences(ref):
    Lm = len(ref.good.centre)
    same_len = 4          # row 4 of `good`: one substitution, as long as the centre
    assert len(ref.seqs[same_len]) == Lm
    bad_streams = {
        "centre advance one short": ([0, same_len], [_op(Lm - 1, "="), _op(1, "D")]),           # member advance Lm: right
        "centre advance long by one op": ([0, same_len], [_op(Lm, "="), _op(1, "I")]),
        "member advance short": ([0, ref.spare_longer], [_op(Lm, "=")]),                        # the member has Lm + 1 bases
        "member advance long": ([0, 2], [_op(Lm, "=")]),                                        # the member has Lm - 1
    }
    for what, (rows, ops) in bad_streams.items():
        rc, n_cols, n_wide, wide = ref.build(rows, ops, [0, 0, len(ops)])
        assert rc == E_ARG and (wide == SENTINEL).all(), what
        assert ref.read_built(2, Lm + 1)[0] == E_ARG, what          # nothing counts as built
        rc, n_cols, n_wide, wide = ref.build_batch([0, 2], rows, ops, [0, 0, len(ops)])
        assert rc == E_ARG and (wide == SENTINEL).all(), what
        ref.still_works()


def test_refused_op_past_the_centre_inside_a_64_op_batch(ref):
    """an '=' run that leaves the centre as op 20 of 100, with insertions into a wide slot behind it: refused by the scan, no record written"""
    r0 = ref.good.n_rows
    rows, ops, ptr = ref.C.single(1)
    assert int(ptr[2]) == 100 and ref.many.host()[1][150] == 4          # row 1 has 100 ops; slot 150 is wide
    bad = ops.copy()
    bad[20] = _op(4000, "=")
    # the wide insertions of rows 2 and 3 stay as they are; row 1 gets one of its own behind the bad op
    bad[60] = _op(3, "D")
    rc, n_cols, n_wide, wide = ref.build(rows, bad, ptr)
    assert rc == E_ARG and n_wide == SENTINEL and (wide == SENTINEL).all()
    rc, n_cols, n_wide, wide = ref.build_batch(ref.C.first_row, ref.C.row_ids, np.concatenate([ref.C.ops[:int(ref.C.ops_ptr[r0])], bad]), ref.C.ops_ptr)
    assert rc == E_ARG and n_wide == SENTINEL and (wide == SENTINEL).all()
    ref.still_works()
    rc, n_cols, n_wide, wide = ref.build(rows, ops, ptr)          # and the same rows with their own ops are accepted
    assert rc == OK and n_wide == 3


def test_refused_arguments_of_the_builds(ref):
    rows, ops, ptr = ref.C.single(0)
    n = len(ref.seqs)
    dec = ptr.copy()
    dec[3] = dec[2] - np.uint64(1)
    assert ref.build(rows, ops, dec)[0] == E_ARG                                   # ops_ptr decreasing
    shifted = ptr.copy()
    shifted[1] = 1
    assert ref.build(rows, ops, shifted)[0] == E_ARG                               # the centre with an op
    out_of_range = rows.copy()
    out_of_range[2] = n
    assert ref.build(out_of_range, ops, ptr)[0] == E_ARG                           # row id out of range
    out_of_range[2], out_of_range[0] = rows[2], n
    assert ref.build(out_of_range, ops, ptr)[0] == E_ARG                           # ... as the centre
    C = ref.C
    assert ref.build_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)[0] == OK
    r0 = int(C.first_row[1])
    assert ref.build_batch([0, r0, r0, C.n_rows], C.row_ids, C.ops, C.ops_ptr)[0] == E_ARG          # a partition without rows
    assert ref.build_batch([0, C.n_rows + 3, C.n_rows], C.row_ids, C.ops, C.ops_ptr)[0] == E_ARG    # ... and one that ends behind the batch
    assert ref.build_batch([1, r0, C.n_rows], C.row_ids, C.ops, C.ops_ptr)[0] == E_ARG
    ids = C.row_ids.copy()
    ids[C.n_rows - 1] = n
    assert ref.build_batch(C.first_row, ids, C.ops, C.ops_ptr)[0] == E_ARG
    dec = C.ops_ptr.copy()
    dec[r0 + 2] = dec[r0 + 1] - np.uint64(1)
    assert ref.build_batch(C.first_row, C.row_ids, C.ops, dec)[0] == E_ARG
    with_op = C.ops_ptr.copy()
    with_op[r0 + 1] += np.uint64(1)                                                # the second centre with an op
    assert ref.build_batch(C.first_row, C.row_ids, C.ops, with_op)[0] == E_ARG
    ref.still_works()


def test_wide_capacity_is_reported_and_the_repeat_succeeds(ref):
    rows, ops, ptr = ref.C.single(0)
    rc, n_cols, n_wide, full = ref.build(rows, ops, ptr, wide_cap=64)
    assert rc == OK and n_wide == 4          # the insertions of rows 1 - 3 into the wide slots 5, 0 and 40
    for cap in (0, n_wide - 1):
        rc, _, need, wide = ref.build(rows, ops, ptr, wide_cap=cap)
        assert rc == E_CAPACITY and need == n_wide and need > cap
        assert ref.read_built(len(rows), n_cols)[0] == E_ARG          # a refused build is no build
        rc, _, got, wide = ref.build(rows, ops, ptr, wide_cap=need)
        assert rc == OK and got == need and sorted_records(wide[:got]) == sorted_records(full[:n_wide])
    C = ref.C
    rc, _, n_all, full = ref.build_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr, wide_cap=64)
    assert rc == OK and n_all == 7
    for cap in (0, n_all - 1):
        rc, _, need, wide = ref.build_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr, wide_cap=cap)
        assert rc == E_CAPACITY and need == n_all and need > cap
        rc, _, got, wide = ref.build_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr, wide_cap=need)
        assert rc == OK and got == need and sorted_records(wide[:got]) == sorted_records(full[:n_all])
    ref.still_works()


def test_packed_capacity_is_reported(ref):
    M, deg = MC.noisy(9, 257, 17, heavy=[(0, 2)])
    p2, o2, n2 = OC.correct_rows(M, deg)
    need = int(o2[-1])
    rc, packed, off, n_cand, tot = correct_abi(M, deg, packed_cap=need - 1)
    assert rc == E_CAPACITY and off[-1] == need and off.tolist() == o2.tolist()
    rc, packed, off, n_cand, tot = correct_abi(M, deg, packed_cap=need)
    assert rc == OK and bytes(packed[:need]) == p2.tobytes()
    # the batch: the built matrices survive the refusal
    C = ref.C
    w = World.__new__(World)
    w.C, w.store, w.single = C, ref.store, {}
    n_cols, slot_base, col_slot, longest, wide = ref.store.msa_build_ops_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)
    pt = batch_patches(w, C.first_row, slot_base, col_slot, longest, wide.copy())
    want = [r for p in C.parts for r in _rows(*OC.correct_rows(p.host()[0], p.deg)[:2])]
    need = sum(len(r) for r in want)
    rc, packed, off, n_cand = ref.correct_built_batch(2, C.n_rows, C.deg, pt, need - 1)
    assert rc == E_CAPACITY and off[-1] == need
    rc, packed, off, n_cand = ref.correct_built_batch(2, C.n_rows, C.deg, pt, need)
    assert rc == OK and _rows(packed, off) == want
    rc, packed, off, n_cand = ref.correct_built_batch(2, C.n_rows, C.deg, pt, need)
    assert rc == E_ARG          # one build serves one correction
    ref.still_works()


def test_refused_patches_shapes_and_repeats(ref):
    rows, ops, ptr = ref.C.single(0)
    nr = len(rows)
    rc, n_cols, n_wide, wide = ref.build(rows, ops, ptr)
    assert rc == OK
    past = (np.array([nr - 1]), np.array([n_cols - 2]), np.array([0, 3]), np.frombuffer(b"ACG", dtype=np.uint8))          # ends one byte past the row
    assert ref.correct_built(nr, n_cols, ref.good.deg, past)[0] == E_ARG
    assert ref.correct_built(nr, n_cols, ref.good.deg, (np.array([nr]), np.array([0]), np.array([0, 1]), np.frombuffer(b"A", dtype=np.uint8)))[0] == E_ARG
    assert ref.read_built(nr, n_cols + 1)[0] == E_ARG and ref.read_built(nr + 1, n_cols)[0] == E_ARG          # another shape than the build's
    rc, M = ref.read_built(nr, n_cols)
    assert rc == OK and (M[0][M[0] != GAP].tobytes().decode() == ref.good.centre)          # the refusals left the build in place
    inside = (np.array([nr - 1]), np.array([n_cols - 3]), np.array([0, 3]), M[nr - 1, n_cols - 3:].copy())            # ends with the row
    assert ref.correct_built(nr, n_cols + 1, ref.good.deg)[0] == E_ARG
    rc, packed, off, n_cand = ref.correct_built(nr, n_cols, ref.good.deg, inside)
    assert rc == OK
    p2, o2, n2 = OC.correct_rows(M, ref.good.deg)
    assert n_cand.tolist() == n2.tolist() and _rows(packed, off) == _rows(p2, o2)
    assert ref.correct_built(nr, n_cols, ref.good.deg)[0] == E_ARG          # one build serves one correction
    assert ref.read_built(nr, n_cols)[0] == E_ARG
    # the batch: a patch that ends one byte past ITS matrix (inside the concatenation)
    C = ref.C
    rc, n_cols_b, n_all, wide = ref.build_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)
    assert rc == OK
    past = (np.array([nr - 1]), np.array([int(n_cols_b[0]) - 2]), np.array([0, 3]), np.frombuffer(b"ACG", dtype=np.uint8))
    assert ref.correct_built_batch(2, C.n_rows, C.deg, past, 1 << 16)[0] == E_ARG
    ref.still_works()


def test_store_with_n_is_refused():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    st = SeqStore(["ACGTNACGT", "ACGTACGT", "ACGTTACGT"])
    try:
        L = _lib.lib()
        rows, ptr, ops = np.arange(2, dtype=np.uint32), np.array([0, 0, 3], dtype=np.uint64), np.array([_op(4, "="), _op(1, "I"), _op(4, "=")], dtype=np.uint32)
        n_cols, n_wide = ctypes.c_uint32(0), ctypes.c_uint64(0)
        buf = np.zeros(64, dtype=np.uint32)
        rc = L.isocon_msa_build_ops(st.handle, 2, _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), ctypes.byref(n_cols), _p(buf, _lib.u32p), _p(buf, _lib.u32p),
                                    _p(buf, _lib.u32p), 1, ctypes.byref(n_wide), None)
        assert rc == E_ALPHABET
        first = np.array([0, 2], dtype=np.uint32)
        n_cols_b = np.zeros(1, dtype=np.uint32)
        rc = L.isocon_msa_build_ops_batch(st.handle, 1, _p(first, _lib.u32p), _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), _p(n_cols_b, _lib.u32p),
                                          _p(buf, _lib.u32p), _p(buf, _lib.u32p), _p(buf, _lib.u32p), 1, ctypes.byref(n_wide), None)
        assert rc == E_ALPHABET
    finally:
        st.close()
