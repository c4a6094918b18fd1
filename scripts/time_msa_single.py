"""The single-partition entry points of the consensus correction (isocon_msa_build_ops + isocon_msa_correct_built, and isocon_msa_correct
on a host matrix) timed on one large partition (a centre of `length` bases with `members` distinct CCS-profile reads of it: the C3 shape)
and on `small` partitions of `small_rows` rows: per call the wall time around the ABI call (each ends in a download) and the call's
kernel_ms; median, min and max of `reps` repeats after a warm-up.  The batched pipeline path is bench.py's; this path serves the repeats
of overflowing partitions and the string path.
--dump file.npz writes every result (packed bytes, offsets, n_cand, class totals); --compare file.npz asserts that this run's results are
bit-equal to such a dump (of another build of the library: the inputs are seeded).
Usage: python scripts/time_msa_single.py [--members 5000] [--length 2500] [--small 200] [--small-rows 10] [--reps 5] [--label text]
                                          [--dump file.npz] [--compare file.npz]"""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from isocon_amd import _lib, synth, correction_module as COR
from isocon_amd.store import SeqStore

ap = argparse.ArgumentParser()
ap.add_argument("--members", type=int, default=5000)
ap.add_argument("--length", type=int, default=2500)
ap.add_argument("--small", type=int, default=200)
ap.add_argument("--small-rows", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--dump", default=None)
ap.add_argument("--compare", default=None)
args = ap.parse_args()
L = _lib.lib()


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def make_partition(rng, n_members):
    centre = synth.make_isoforms(rng, args.length, 1)[0]
    seqs, seen = [centre.tobytes().decode()], set()
    while len(seqs) < 1 + n_members:
        s = synth.mutate(rng, centre, synth.CCS_PROFILE).tobytes().decode()
        if s not in seen and s != seqs[0]:
            seen.add(s)
            seqs.append(s)
    return seqs


def rows_and_ops(st, first, n_rows):
    """rows first .. first + n_rows of the store as a partition: (row ids, ops, ops_ptr) with the members' alignments against the centre"""
    a = np.full(n_rows - 1, first, dtype=np.uint32)
    b = np.arange(first + 1, first + n_rows, dtype=np.uint32)
    ops, ptr, _ = st.sg_trace(a, b, -2, ed_upper=st.ed_pairs(a, b, None))
    return np.arange(first, first + n_rows, dtype=np.uint32), ops.copy(), np.concatenate([[0], ptr]).astype(np.uint64)


def build(st, rows, ops, ptr):
    """isocon_msa_build_ops -> (n_cols, col_slot, longest, wide, wall s, kernel ms)"""
    Lm = int(st.lens[int(rows[0])])
    n_cols, n_wide, ms = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_float(0)
    col_slot, longest = np.zeros(Lm + 1, dtype=np.uint32), np.zeros(Lm + 1, dtype=np.uint32)
    wide = np.empty((max(1 << 16, 8 * len(rows)), 8), dtype=np.uint32)
    t0 = time.perf_counter()
    rc = L.isocon_msa_build_ops(st.handle, len(rows), _p(rows, _lib.u32p), _p(ops, _lib.u32p), _p(ptr, _lib.u64p), ctypes.byref(n_cols), _p(col_slot, _lib.u32p),
                                _p(longest, _lib.u32p), _p(wide, _lib.u32p), len(wide), ctypes.byref(n_wide), ctypes.byref(ms))
    wall = time.perf_counter() - t0
    _lib.check(rc, "isocon_msa_build_ops")
    return int(n_cols.value), col_slot, longest, wide[:int(n_wide.value)].copy(), wall, ms.value


def correct_built(st, n_rows, n_cols, deg, pt):
    n_p = 0 if pt[0] is None else len(pt[0])
    arrs = [None if not n_p else np.ascontiguousarray(x, dtype=t) for x, t in zip(pt, (np.uint32, np.uint32, np.uint32, np.uint8))]
    packed, off, n_cand = np.empty(n_rows * n_cols, dtype=np.uint8), np.zeros(n_rows + 1, dtype=np.uint64), np.zeros(n_rows, dtype=np.int32)
    tot, ms = (ctypes.c_int64 * 3)(), ctypes.c_float(0)
    t0 = time.perf_counter()
    rc = L.isocon_msa_correct_built(st.handle, n_rows, n_cols, _p(arrs[0], _lib.u32p), _p(arrs[1], _lib.u32p), _p(arrs[2], _lib.u32p), _p(arrs[3], _lib.u8p), n_p,
                                    _p(deg, _lib.i32p), _p(packed, _lib.u8p), packed.size, _p(off, _lib.u64p), _p(n_cand, _lib.i32p), tot, ctypes.byref(ms))
    wall = time.perf_counter() - t0
    _lib.check(rc, "isocon_msa_correct_built")
    return (packed[:int(off[-1])].copy(), off.astype(np.int64), n_cand, np.array(list(tot), dtype=np.int64)), wall, ms.value


def correct_host(M, deg):
    nr, ncols = M.shape
    packed, off, n_cand = np.empty(M.size, dtype=np.uint8), np.zeros(nr + 1, dtype=np.uint64), np.zeros(nr, dtype=np.int32)
    tot, ms = (ctypes.c_int64 * 3)(), ctypes.c_float(0)
    t0 = time.perf_counter()
    rc = L.isocon_msa_correct(_p(M, _lib.u8p), nr, ncols, _p(deg, _lib.i32p), _p(packed, _lib.u8p), packed.size, _p(off, _lib.u64p), _p(n_cand, _lib.i32p), tot,
                              ctypes.byref(ms))
    wall = time.perf_counter() - t0
    _lib.check(rc, "isocon_msa_correct")
    return (packed[:int(off[-1])].copy(), off.astype(np.int64), n_cand, np.array(list(tot), dtype=np.int64)), wall, ms.value


def run_partitions(st, parts, seqs):
    """every partition through build + correct_built and through isocon_msa_correct on the same (patched) matrix, one after the other ->
    (results (the two paths agree), [build wall, build kernel, correct wall, correct kernel, host-matrix wall, host-matrix kernel] sums)"""
    res_a, sums = [], np.zeros(6)
    for rows, ops, ptr, deg in parts:
        n_cols, col_slot, longest, wide, w1, k1 = build(st, rows, ops, ptr)
        M = st.msa_read_built(len(rows), n_cols)
        pt = COR._wide_slot_patches([seqs[int(r)] for r in rows[1:]], wide, col_slot, longest)
        for k in range(0 if pt[0] is None else len(pt[0])):
            M[pt[0][k], pt[1][k]:pt[1][k] + int(pt[2][k + 1] - pt[2][k])] = pt[3][int(pt[2][k]):int(pt[2][k + 1])]
        ra, w2, k2 = correct_built(st, len(rows), n_cols, deg, pt)
        rb, w3, k3 = correct_host(M, deg)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), "the two single-partition paths differ"
        res_a.append(ra)
        sums += [w1, k1, w2, k2, w3, k3]
    return res_a, sums


def timed(name, st, parts, seqs, out):
    run_partitions(st, parts[:1], seqs)          # warm-up: scratch slots, code objects
    reps = []
    for _ in range(args.reps):
        res, sums = run_partitions(st, parts, seqs)
        reps.append(sums)
    reps = np.array(reps)
    reps[:, [0, 2, 4]] *= 1e3
    for j, what in enumerate(("build_ops wall", "build_ops kernels", "correct_built wall", "correct_built kernels", "msa_correct wall", "msa_correct kernels")):
        out["%s %s ms" % (name, what)] = [round(float(np.median(reps[:, j])), 3), round(float(reps[:, j].min()), 3), round(float(reps[:, j].max()), 3)]
    return res


rng = np.random.Generator(np.random.PCG64(2024))
out = {"label": args.label, "members": args.members, "length": args.length, "small": args.small, "small_rows": args.small_rows, "reps": args.reps,
       "columns": "median, min, max"}
dump = {}
# one large partition
seqs = make_partition(rng, args.members)
st = SeqStore(seqs)
rows, ops, ptr = rows_and_ops(st, 0, len(seqs))
deg = np.ones(len(seqs), dtype=np.int32)
deg[0] = 3
res = timed("large", st, [(rows, ops, ptr, deg)], seqs, out)
for name, x in zip(("packed", "off", "n_cand", "tot"), res[0]):
    dump["large_" + name] = x
st.close()
# many small ones, in one store
seqs = []
for _ in range(args.small):
    seqs += make_partition(rng, args.small_rows - 1)
st = SeqStore(seqs)
parts = []
deg = np.ones(args.small_rows, dtype=np.int32)
deg[0] = 2
for i in range(args.small):
    parts.append(rows_and_ops(st, i * args.small_rows, args.small_rows) + (deg,))
res = timed("small (sum of %d)" % args.small, st, parts, seqs, out)
for j, name in enumerate(("packed", "off", "n_cand", "tot")):
    dump["small_" + name] = np.concatenate([r[j] for r in res])
st.close()
if args.dump:
    np.savez(args.dump, **dump)
if args.compare:
    want = np.load(args.compare)
    for k in sorted(dump):
        assert np.array_equal(dump[k], want[k]), "%s differs from %s" % (k, args.compare)
    out["bit_equal_to"] = os.path.basename(args.compare)
print(json.dumps(out), flush=True)
