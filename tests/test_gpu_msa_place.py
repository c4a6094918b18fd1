"""The placed builds (isocon_msa_build_ops_placed[_batch]: the insertions of the wide slots placed on the device, csrc/msa_place_core.hpp,
k_msa_slot_rep / k_msa_place of csrc/msa.hpp) against the host matrix (functions.msa_matrix, which places them with
functions.get_best_solution) on the designed partitions of tests/msa_place_cases.py; the corrected rows against the numpy checker
(oracle/correction.py); the route of correction_module with its switch; the refusals.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import msa_cases as MC
import msa_place_cases as PC
from oracle import correction as OC

pytestmark = pytest.mark.gpu

OK, E_ARG, E_ALPHABET, E_CAPACITY = 0, -1, -2, -4


def _p(a, t):
    return a.ctypes.data_as(t)


def _rows(packed, off):
    return [bytes(packed[int(off[r]):int(off[r + 1])]) for r in range(len(off) - 1)]


class World(object):
    def __init__(self):
        from isocon_amd.store import SeqStore
        self.P, self.plan = PC.build_partitions()
        self.parts = [self.P[k] for k in PC.ORDER]
        self.C = MC.Concatenation(self.parts)
        self.store = SeqStore(list(self.C.seqs))
        self.expected = [OC.correct_rows(p.host()[0], p.deg) for p in self.parts]          # once, for the single and the batched test

    def records(self, i):
        """(records in slots the device places, records in slots left to the host) of partition i, from its gapped strings"""
        p, longest = self.parts[i], self.parts[i].host()[1]
        wide = [(r, t, s) for r, t, s in p.insertions() if longest[t] > 1]
        return [x for x in wide if longest[x[1]] <= PC.CAP], [x for x in wide if longest[x[1]] > PC.CAP]


def host_patches(part, left, col_slot, longest):
    from isocon_amd import correction_module as COR
    return COR._wide_slot_patches(part.members, left, col_slot, longest)


def apply_patches(M, pt):
    for k in range(0 if pt[0] is None else len(pt[0])):
        M[pt[0][k], pt[1][k]:pt[1][k] + int(pt[2][k + 1] - pt[2][k])] = pt[3][int(pt[2][k]):int(pt[2][k + 1])]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.store.close()


@pytest.mark.parametrize("i", range(len(PC.ORDER)), ids=PC.ORDER)
def test_placed_matrix_equals_host_matrix(world, i):
    st, p = world.store, world.parts[i]
    host, longest_h, col_slot_h = p.host()
    rows, ops, ptr = world.C.single(i)
    n_wide = len(st.msa_build_ops(rows, ops, ptr)[3])          # the record count of the build that lists them all
    n_cols, col_slot, longest, left, n_placed = st.msa_build_ops_placed(rows, ops, ptr)
    placed_h, left_h = world.records(i)
    print("%s: %d records placed, %d left" % (p.name, n_placed, len(left)))
    assert n_cols == host.shape[1] and col_slot.tolist() == col_slot_h.tolist() and longest.tolist() == longest_h.tolist()
    assert n_placed == len(placed_h) and len(left) == len(left_h) and n_placed + len(left) == n_wide
    assert sorted((int(r), int(t), int(n)) for r, t, _, n in left[:, :4].tolist()) == sorted((r, t, len(s)) for r, t, s in left_h)
    assert {t for _, t, _ in left_h} == {t for t, what in world.plan[p.name].items() if what == "left"}
    assert {t for _, t, _ in placed_h} >= {t for t, what in world.plan[p.name].items() if what == "placed"}
    dev = st.msa_read_built(p.n_rows, n_cols)
    if left_h:          # without the host's patches exactly the left slots are still empty in the members' rows
        for t in {t for _, t, _ in left_h}:
            c0 = int(col_slot[t])
            assert (dev[:, c0:c0 + int(longest[t]) + 2] == 45).all()
    pt = host_patches(p, left.copy(), col_slot, longest)
    apply_patches(dev, pt)
    assert dev.shape == host.shape
    assert (dev == host).all(), np.argwhere(dev != host)[:5].tolist()
    packed, off, n_cand = st.msa_correct_built(p.n_rows, n_cols, p.deg, *pt)
    p2, o2, n2 = world.expected[i]
    assert n_cand.tolist() == n2.tolist() and off.tolist() == o2.tolist() and bytes(packed[:off[-1]]) == p2.tobytes()


def test_placed_batch_equals_host(world):
    C, st = world.C, world.store
    n_wide = len(st.msa_build_ops_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)[4])
    n_cols, slot_base, col_slot, longest, left, n_placed = st.msa_build_ops_placed_batch(C.first_row, C.row_ids, C.ops, C.ops_ptr)
    placed_h = sum(len(world.records(i)[0]) for i in range(len(C.parts)))
    left_h = sum(len(world.records(i)[1]) for i in range(len(C.parts)))
    assert n_placed == placed_h and len(left) == left_h > 0 and n_placed + len(left) == n_wide
    assert set(left[:, 6].tolist()) == {PC.ORDER.index("lengths")}
    rows_l, cols_l, lens_l, bytes_l = [], [], [], []
    for i in sorted(set(left[:, 6].tolist())):
        local = left[left[:, 6] == i].copy()
        r0, sb, se = int(C.first_row[i]), int(slot_base[i]), int(slot_base[i + 1])
        local[:, 0] -= r0
        pr, pc, pp, pb = host_patches(C.parts[i], local, col_slot[sb:se], longest[sb:se])
        rows_l.append(np.asarray(pr, dtype=np.int64) + r0); cols_l.append(np.asarray(pc, dtype=np.int64)); lens_l.append(np.diff(pp.astype(np.int64))); bytes_l.append(pb)
    p_ptr = np.zeros(sum(len(x) for x in rows_l) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(lens_l), out=p_ptr[1:])
    cap = int(sum(len(s) for s in C.seqs)) + 16 * C.n_rows + 1024
    packed, off, n_cand = st.msa_correct_built_batch(len(C.parts), C.n_rows, C.deg, cap, np.concatenate(rows_l), np.concatenate(cols_l), p_ptr, np.concatenate(bytes_l))
    rows = _rows(packed, off)
    for i, p in enumerate(C.parts):
        host, longest_h, col_slot_h = p.host()
        r0, r1, sb, se = int(C.first_row[i]), int(C.first_row[i + 1]), int(slot_base[i]), int(slot_base[i + 1])
        assert n_cols[i] == host.shape[1] and col_slot[sb:se].tolist() == col_slot_h.tolist() and longest[sb:se].tolist() == longest_h.tolist()
        p2, o2, n2 = world.expected[i]
        assert n_cand[r0:r1].tolist() == n2.tolist(), p.name
        assert rows[r0:r1] == _rows(p2, o2), p.name


# ---- correction_module ------------------------------------------------------------------------------------------------------------------------

class Params(object):
    nr_cores = 1
    neighbor_search_depth = 2 ** 32
    verbose = False
    develop_logfile = None
    min_exon_diff = 20
    ignore_ends_len = 15


@pytest.fixture(scope="module")
def ont_step():
    from isocon_amd import isocon_get_candidates as IGC
    from isocon_amd import partitions, synth
    accs, seqs, _ = synth.make_reads(400, 500, 3, seed=63, profile=synth.ONT_PROFILE)
    S = dict(zip(accs, seqs))
    G, partition, M, converged = partitions.partition_strings(S, Params())
    pa = IGC.get_partition_alignments(partition, M, G, set(), Params())
    assert pa.batch is not None and pa.batch.alive()
    return pa, IGC.get_unique_seq_accessions(S)


def test_correct_strings_equal_on_both_routes(ont_step, monkeypatch):
    from isocon_amd import correction_module as COR
    pa, seq_to_acc = ont_step
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    before = dict(COR.PLACE_STATS)
    dev, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
    after = dict(COR.PLACE_STATS)
    assert after["calls"] > before["calls"] and after["placed"] - before["placed"] > 50
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "msa_host_place")
    host, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
    assert COR.PLACE_STATS == after          # nothing placed, no placed build
    assert dev == host and len(dev) > 100
    # one partition at a time: the single-partition placed build
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT")
    m = max(pa, key=lambda k: len(pa[k]))
    one = COR._correct_partition_from_ops(pa.batch, m, pa[m], seq_to_acc)
    assert COR.PLACE_STATS["calls"] == after["calls"] + 1 and COR.PLACE_STATS["placed"] > after["placed"]
    monkeypatch.setenv("ISOCON_DEBUG_VARIANT", "msa_host_place")
    assert one == COR._correct_partition_from_ops(pa.batch, m, pa[m], seq_to_acc) and len(one) > 10


class OldStore(object):
    """a store object from before the placed builds: the four methods the host route needs, and nothing else"""

    def __init__(self, store):
        self._h, self.lens = store._h, store.lens
        self.msa_build_ops, self.msa_correct_built = store.msa_build_ops, store.msa_correct_built
        self.msa_build_ops_batch, self.msa_correct_built_batch = store.msa_build_ops_batch, store.msa_correct_built_batch


def test_a_store_without_the_placed_builds_takes_the_host_route(ont_step, monkeypatch):
    from isocon_amd import correction_module as COR
    pa, seq_to_acc = ont_step
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    want, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
    real = pa.batch.store
    before = dict(COR.PLACE_STATS)
    pa.batch.store = OldStore(real)
    try:
        got, _ = COR.correct_strings(pa, seq_to_acc, {}, 1)
    finally:
        pa.batch.store = real
    assert COR.PLACE_STATS == before and got == want


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------

def placed_abi(st, C, i, left_cap, batch=False):
    """the raw entry points on partition i (batch: on all partitions) -> (rc, n_cols, n_left, n_placed, left)"""
    from isocon_amd import _lib
    L = _lib.lib()
    n_left, n_placed = ctypes.c_uint64(12345), ctypes.c_uint64(12345)
    left = np.full((max(left_cap, 1), 8), 0xA5A5A5A5, dtype=np.uint32)
    if batch:
        first = np.ascontiguousarray(C.first_row, dtype=np.uint32)
        rows, ops, ptr = C.row_ids, C.ops, C.ops_ptr
        n_slots = int(sum(len(p.centre) + 1 for p in C.parts))
        n_cols = np.zeros(len(C.parts), dtype=np.uint32)
    else:
        rows, ops, ptr = C.single(i)
        n_slots = len(C.parts[i].centre) + 1
        n_cols = np.zeros(1, dtype=np.uint32)
    rows, ops, ptr = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(ops, dtype=np.uint32), np.ascontiguousarray(ptr, dtype=np.uint64)
    col_slot, longest = np.zeros(n_slots, dtype=np.uint32), np.zeros(n_slots, dtype=np.uint32)
    if batch:
        rc = L.isocon_msa_build_ops_placed_batch(st.handle, len(C.parts), _p(first, _lib.u32p), _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), _p(n_cols, _lib.u32p),
                                                 _p(col_slot, _lib.u32p), _p(longest, _lib.u32p), _p(left, _lib.u32p), left_cap, ctypes.byref(n_left), ctypes.byref(n_placed), None)
    else:
        rc = L.isocon_msa_build_ops_placed(st.handle, len(rows), _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), _p(n_cols, _lib.u32p), _p(col_slot, _lib.u32p),
                                           _p(longest, _lib.u32p), _p(left, _lib.u32p), left_cap, ctypes.byref(n_left), ctypes.byref(n_placed), None)
    return rc, n_cols, int(n_left.value), int(n_placed.value), left


def test_left_capacity_is_reported_and_the_build_stays(world):
    st, C = world.store, world.C
    i = PC.ORDER.index("lengths")
    p = C.parts[i]
    want = len(world.records(i)[1])
    assert want == 15          # five rows in each of the slots of 63, 64 and 70 bases
    for cap in (0, want - 1):
        rc, n_cols, n_left, n_placed, left = placed_abi(st, C, i, cap)
        assert rc == E_CAPACITY and n_left == want and n_placed == len(world.records(i)[0])
        first = st.msa_read_built(p.n_rows, int(n_cols[0]))          # the build stays
        rc, n_cols2, n_left2, n_placed2, left = placed_abi(st, C, i, n_left)
        assert rc == OK and (n_left2, n_placed2, n_cols2.tolist()) == (n_left, n_placed, n_cols.tolist())
        assert (st.msa_read_built(p.n_rows, int(n_cols[0])) == first).all()
        assert sorted(left[:, 1].tolist()) == sorted(t for _, t, _ in world.records(i)[1])
    rc, n_cols, n_left, n_placed, left = placed_abi(st, C, 0, 0, batch=True)
    assert rc == E_CAPACITY and n_left == want
    rc, n_cols, n_left, n_placed, left = placed_abi(st, C, 0, want, batch=True)
    assert rc == OK and n_left == want and set(left[:, 6].tolist()) == {i}


def test_single_and_batch_still_pair_with_their_own_kind(world):
    from isocon_amd import _lib
    st, C = world.store, world.C
    L = _lib.lib()
    i = PC.ORDER.index("twin_a")
    p = C.parts[i]
    rc, n_cols, n_left, n_placed, left = placed_abi(st, C, i, 16)
    assert rc == OK and n_left == 0 and n_placed == 3
    deg = np.ascontiguousarray(p.deg, dtype=np.int32)
    packed, off, n_cand = np.zeros(1 << 16, dtype=np.uint8), np.zeros(p.n_rows + 1, dtype=np.uint64), np.zeros(p.n_rows, dtype=np.int32)
    rc = L.isocon_msa_correct_built_batch(st.handle, 1, p.n_rows, None, None, None, None, 0, _p(deg, _lib.i32p), _p(packed, _lib.u8p), packed.size, _p(off, _lib.u64p),
                                          _p(n_cand, _lib.i32p), None)
    assert rc == E_ARG
    assert (st.msa_read_built(p.n_rows, int(n_cols[0])) == p.host()[0]).all()          # the refusal left the single build in place
    rc, n_cols_b, n_left, n_placed, left = placed_abi(st, C, 0, 64, batch=True)
    assert rc == OK
    M = np.zeros((C.parts[0].n_rows, int(n_cols_b[0])), dtype=np.uint8)
    assert L.isocon_msa_read_built(st.handle, C.parts[0].n_rows, int(n_cols_b[0]), _p(M, _lib.u8p)) == E_ARG
    deg0 = np.ascontiguousarray(C.parts[0].deg, dtype=np.int32)
    off0, n_cand0 = np.zeros(C.parts[0].n_rows + 1, dtype=np.uint64), np.zeros(C.parts[0].n_rows, dtype=np.int32)
    rc = L.isocon_msa_correct_built(st.handle, C.parts[0].n_rows, int(n_cols_b[0]), None, None, None, None, 0, _p(deg0, _lib.i32p), _p(packed, _lib.u8p), packed.size,
                                    _p(off0, _lib.u64p), _p(n_cand0, _lib.i32p), None, None)
    assert rc == E_ARG


def test_store_over_another_alphabet_is_refused():
    from isocon_amd import _lib
    from isocon_amd.store import SeqStore
    st = SeqStore(["ACGTNACGT", "ACGTACGT", "ACGTTACGT"])
    try:
        L = _lib.lib()
        rows, ptr = np.arange(2, dtype=np.uint32), np.array([0, 0, 3], dtype=np.uint64)
        ops = np.array([(4 << 4) | 0, (1 << 4) | 2, (4 << 4) | 0], dtype=np.uint32)
        n_cols, n_left, n_placed = np.zeros(1, dtype=np.uint32), ctypes.c_uint64(0), ctypes.c_uint64(0)
        buf = np.zeros(64, dtype=np.uint32)
        rc = L.isocon_msa_build_ops_placed(st.handle, 2, _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), _p(n_cols, _lib.u32p), _p(buf, _lib.u32p),
                                           _p(buf, _lib.u32p), _p(buf, _lib.u32p), 1, ctypes.byref(n_left), ctypes.byref(n_placed), None)
        assert rc == E_ALPHABET
        first = np.array([0, 2], dtype=np.uint32)
        rc = L.isocon_msa_build_ops_placed_batch(st.handle, 1, _p(first, _lib.u32p), _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), _p(n_cols, _lib.u32p),
                                                 _p(buf, _lib.u32p), _p(buf, _lib.u32p), _p(buf, _lib.u32p), 1, ctypes.byref(n_left), ctypes.byref(n_placed), None)
        assert rc == E_ALPHABET
    finally:
        st.close()
