"""CPU: the base-quality lane math of the device read tables (isocon_amd/csrc/readtab_core.hpp: rt_read_bases_upto, rt_quality_code)
driven by 64 emulated lanes (tests/emul/readtab_quality_emul.cpp, g++ and UBSan) in the shape of k_rt_read_prefix / k_rt_quality:
the read rows' gap masks and prefix counts against the strings, the read bases up to a column against _ReadTable.read_bases_upto, and
the code bytes against a direct restatement of functions._ccs_probabilities (tests/readtab_quality_cases.py) and against the host
tables, on directed and random cases and on the reference's fixture g16."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_quality_cases as QC  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

SO = os.path.join(HERE, "emul", "_readtab_quality_emul.so")
SRCS = [os.path.join(HERE, "emul", f) for f in ("readtab_quality_emul.cpp", "readtab_emul.cpp")]
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "readtab_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def emul(request):
    so = SO if request.param == "plain" else SO.replace(".so", "_ubsan.so")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-static-libubsan"]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in SRCS + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRCS[0]])
    L = ctypes.CDLL(so)
    L.rt_emul_build.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    L.rt_emul_read_prefix.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 2
    L.rt_emul_read_prefix.restype = None
    L.rt_emul_read_bases_upto.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    L.rt_emul_read_bases_upto.restype = ctypes.c_int64
    L.rt_emul_quality.argtypes = [ctypes.c_void_p] * 12 + [ctypes.c_uint32] + [ctypes.c_void_p] * 10
    L.rt_emul_quality.restype = None
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _pad(a):
    return a if len(a) else np.zeros(1, a.dtype)


def build(L, items, ccs_dict=None):
    """the emulated k_rt_build and k_rt_read_prefix over a table set, with the records of ccs_dict as isocon_readtab_set_qualities takes them"""
    ref, read, row_ptr, first_row = H._pack_rows(items)
    n = len(row_ptr) - 1
    blk_ptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum((np.diff(row_ptr) + np.uint64(63)) // np.uint64(64), out=blk_ptr[1:])
    nb = int(blk_ptr[-1])
    T = dict(read=_pad(read), row_ptr=row_ptr, blk_ptr=blk_ptr, first_row=first_row, nob=np.zeros(nb + 1, np.uint64), diff=np.zeros(nb + 1, np.uint64),
             pre=np.zeros(nb + 1, np.uint32), out=np.zeros((n + 1, 4), np.uint32), rgap=np.full(nb + 1, 7, np.uint64), rpre=np.full(nb + 1, 7, np.uint32))
    assert L.rt_emul_build(_p(_pad(ref)), _p(T["read"]), _p(row_ptr), _p(blk_ptr), n, _p(T["nob"]), _p(T["diff"]), _p(T["pre"]), _p(T["out"])) == 0
    L.rt_emul_read_prefix(_p(T["read"]), _p(row_ptr), _p(blk_ptr), n, _p(T["rgap"]), _p(T["rpre"]))
    if ccs_dict is not None:
        rows = [(acc, v[1]) for _, ra in items for acc, v in ra.items()]
        recs = [ccs_dict[acc] for acc, _ in rows]
        T["qual"] = _pad(np.asarray([q for r in recs for q in r.qual], dtype=np.uint8))
        T["qual_ptr"] = np.asarray(np.cumsum([0] + [len(r.qual) for r in recs]), dtype=np.uint64)
        T["rec_start"] = _pad(np.asarray([r.seq.index(row.replace("-", "")) for r, (_, row) in zip(recs, rows)], dtype=np.uint32))
    return T


def check_read_masks(T, items):
    """rgap / rpre of every block against the strings"""
    r = 0
    for _, ra in items:
        for _, b, _ in ra.values():
            blk0 = int(T["blk_ptr"][r])
            bases = 0
            for blk in range((len(b) + 63) // 64):
                cols = range(blk * 64, min(len(b), blk * 64 + 64))
                assert (int(T["rgap"][blk0 + blk]), int(T["rpre"][blk0 + blk])) == (sum(1 << (j - blk * 64) for j in cols if b[j] == "-"), bases), (r, blk)
                bases += sum(1 for j in cols if b[j] != "-")
            r += 1
    assert int(T["rgap"][int(T["blk_ptr"][-1])]) == 7          # nothing written past the last block


def quality(L, T, items, queries):
    """the emulated k_rt_quality: per query the (variants, reads) code bytes"""
    q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, _ = H._pack_queries(QC.with_rows(items, queries))
    ref_len_of_var = np.repeat(np.asarray([items[k][0] for k in q_table.tolist()], dtype=np.int64), np.diff(var_ptr).astype(np.int64))
    pos = np.where(var_pos < 0, var_pos + ref_len_of_var, var_pos).astype(np.uint32)          # (what the host entry does before the launch)
    sizes = [len(coords) * len(items[k][1]) for k, _, coords, _ in queries]
    code_ptr = np.asarray(np.cumsum([0] + sizes), dtype=np.uint64)
    codes = np.full(int(code_ptr[-1]) + 1, 0xAB, np.uint8)
    L.rt_emul_quality(_p(T["row_ptr"]), _p(T["blk_ptr"]), _p(T["nob"]), _p(T["diff"]), _p(T["pre"]), _p(T["read"]), _p(T["first_row"]), _p(T["rgap"]), _p(T["rpre"]),
                      _p(T["qual"]), _p(T["qual_ptr"]), _p(T["rec_start"]), len(queries), _p(_pad(q_table)), _p(_pad(q_kind)), _p(var_ptr), _p(_pad(pos)), _p(_pad(var_u)),
                      _p(_pad(var_type)), _p(snip_ptr), _p(snip_bytes), _p(code_ptr), _p(codes))
    assert codes[-1] == 0xAB
    return [codes[int(code_ptr[q]):int(code_ptr[q + 1])].reshape(len(coords), len(items[k][1])) for q, (k, _, coords, _) in enumerate(queries)]


def check_case(L, items, queries, ccs):
    T = build(L, items, ccs)
    check_read_masks(T, items)
    got = quality(L, T, items, queries)
    want = QC.expected_codes(items, queries, ccs)
    host = QC.table_codes(items, queries, ccs)
    for q in range(len(queries)):
        assert np.array_equal(got[q], want[q]), (q, queries[q], got[q].tolist(), want[q].tolist())
        assert np.array_equal(host[q], want[q]), (q, queries[q], host[q].tolist(), want[q].tolist())
    return np.concatenate([g.ravel() for g in got]) if got else np.zeros(0, np.uint8)


def test_read_bases_upto(emul):
    """every column of rows of length 1, 63, 64, 65, 128, 129 and 200 -- one of them a read row that opens with more than 64 gap columns
    -- against _ReadTable.read_bases_upto and the string"""
    rng = random.Random(3)
    ra = {}
    for n in (1, 63, 64, 65, 128, 129, 200):
        for style in range(3):
            c = "".join(rng.choice("ACGT") for _ in range(n))
            b = "".join("-" if rng.random() < (0.0, 0.1, 0.5)[style] else ch for ch in c)
            ra["n%d_%d" % (n, style)] = (c, b, ())
    c = "".join(rng.choice("ACGT") for _ in range(200))
    ra["lead"] = (c, "-" * 70 + c[70:], ())
    ra["all_gaps"] = (c[:130], "-" * 130, ())
    items = [(0, ra)]          # (ref_len is not looked at here)
    T = build(emul, items)
    check_read_masks(T, items)
    tab = H._ReadTable(0, ra)
    longest = max(len(v[1]) for v in ra.values())
    upto = [tab.read_bases_upto(np.full(tab.n, pos, dtype=np.int64)) for pos in range(longest)]
    for r, (_, b, _) in enumerate(ra.values()):
        blk0 = int(T["blk_ptr"][r])
        for pos in range(len(b)):
            got = emul.rt_emul_read_bases_upto(_p(T["rgap"][blk0:]), _p(T["rpre"][blk0:]), pos)
            assert got == pos + 1 - b.count("-", 0, pos + 1) == int(upto[pos][r]), (r, pos)


def test_directed_shapes(emul):
    items, queries, ccs, marks = QC.directed_case()
    codes = check_case(emul, items, queries, ccs)
    want = QC.expected_codes(items, queries, ccs)
    at = lambda name: [int(want[q][v, j]) for q, v, j in marks[name]]  # noqa: E731
    assert at("seen_0") == [93, 93] and at("coord_is_rec_len") == [0] and at("beyond") == [QC.Q_BEYOND] and at("index") == [QC.Q_INDEX]
    assert at("both") == [QC.Q_BOTH] * 2 and at("quality_0") == [0] and at("quality_93") == [93]
    counts = {c: int((codes == c).sum()) for c in (QC.Q_INDEX, QC.Q_BEYOND, QC.Q_BOTH, QC.Q_NEITHER)}
    assert all(counts.values()) and int((codes <= 93).sum()) > 500, counts


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(emul, seed):
    items, queries, ccs = QC.random_case(seed)
    codes = check_case(emul, items, queries, ccs)
    assert int((codes <= 93).sum()) > 50 and int((codes == QC.Q_NEITHER).sum()) > 10 and int((codes == QC.Q_BOTH).sum()) > 0


def test_reference_fixture(emul):
    """fixture g16: the code bytes lead to the reference's own probabilities and non-informative reads"""
    n_prob = n_non = 0
    for items, (vt, vc, ac2t, at2c), ccs, want_c, want_t in QC.g16_quality_cases():
        queries = [(0, 0, vc, at2c), (1, 1, vt, ac2t)]
        T = build(emul, items, ccs)
        got = quality(emul, T, items, queries)
        errors = T["out"][:len(T["row_ptr"]) - 1, :3].astype(np.int64)
        sums = [float(max(1.0, int(errors[:, e].sum()))) for e in (2, 0, 1)]          # substitutions, insertions, deletions
        ratios = tuple(x / sum(sums) for x in sums)
        for side, coords, want in ((0, vc, want_c), (1, vt, want_t)):
            accs = list(items[side][1])
            alive, prob = H._ccs_probabilities_from_codes(len(accs), coords, lambda v, *_: got[side][v], ratios, 43)
            assert [[a, repr(float(p))] for a, p, ok in zip(accs, prob, alive) if ok] == want[0]
            assert sorted(a for a, ok in zip(accs, alive) if not ok) == sorted(want[1])
            n_prob += len(want[0])
            n_non += len(want[1])
    assert (n_prob, n_non) == (527, 21 + 12)          # the fixture's non-informative reads: 21 of c, 12 of t
