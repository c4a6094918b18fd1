"""CPU: the lane math of the device read tables (isocon_amd/csrc/readtab_core.hpp, shared host/device header) driven by 64 emulated
lanes (tests/emul/readtab_emul.cpp, g++ and UBSan) in the shape of k_rt_build / k_rt_support: masks, prefix counts, error counts
and query bits against hypothesis_test_module._ReadTable / functions.read_errors_from_alignment on directed and random rows."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_cases as RC  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

SO = os.path.join(HERE, "emul", "_readtab_emul.so")
SRC = os.path.join(HERE, "emul", "readtab_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "readtab_core.hpp")]
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", params=["plain", "ubsan"])
def emul(request):
    so = SO if request.param == "plain" else SO.replace(".so", "_ubsan.so")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-static-libubsan"]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.rt_emul_select_zero.argtypes = [ctypes.c_uint64, ctypes.c_int]
    L.rt_emul_window.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
    L.rt_emul_window.restype = ctypes.c_uint64
    L.rt_emul_range_mask.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.rt_emul_range_mask.restype = ctypes.c_uint64
    L.rt_emul_find_block.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    L.rt_emul_find_block.restype = ctypes.c_uint32
    L.rt_emul_lead_ones.argtypes = [ctypes.c_uint64, ctypes.c_int]
    L.rt_emul_trail_ones.argtypes = [ctypes.c_uint64, ctypes.c_int]
    L.rt_emul_build.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    L.rt_emul_support.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint32] + [ctypes.c_void_p] * 11
    L.rt_emul_support.restype = None
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def build(L, items):
    """the emulated k_rt_build over a table set"""
    ref, read, row_ptr, first_row = H._pack_rows(items)
    n = len(row_ptr) - 1
    blk_ptr = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum((np.diff(row_ptr) + np.uint64(63)) // np.uint64(64), out=blk_ptr[1:])
    nb = int(blk_ptr[-1])
    T = dict(ref=ref, read=read if len(read) else np.zeros(1, np.uint8), row_ptr=row_ptr, blk_ptr=blk_ptr, first_row=first_row, nob=np.zeros(nb + 1, np.uint64),
             diff=np.zeros(nb + 1, np.uint64), pre=np.zeros(nb + 1, np.uint32), out=np.zeros((n + 1, 4), np.uint32))
    refp = ref if len(ref) else np.zeros(1, np.uint8)
    T["bad"] = L.rt_emul_build(_p(refp), _p(T["read"]), _p(row_ptr), _p(blk_ptr), n, _p(T["nob"]), _p(T["diff"]), _p(T["pre"]), _p(T["out"]))
    T["out"] = T["out"][:n]
    return T


def support(L, T, items, queries):
    """the emulated k_rt_support: supporting row indices per query"""
    q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, bits_ptr = H._pack_queries(RC.with_rows(items, queries))
    ref_len_of_var = np.repeat(np.asarray([items[k][0] for k in q_table.tolist()], dtype=np.int64), np.diff(var_ptr).astype(np.int64))
    pos = np.where(var_pos < 0, var_pos + ref_len_of_var, var_pos).astype(np.uint32)          # (what the host entry does before the launch)
    bits = np.zeros(int(bits_ptr[-1]) + 1, np.uint64)
    count = np.zeros(len(queries) + 1, np.uint32)
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    L.rt_emul_support(_p(T["row_ptr"]), _p(T["blk_ptr"]), _p(T["nob"]), _p(T["diff"]), _p(T["pre"]), _p(T["read"]), _p(T["first_row"]), len(queries), _p(pad(q_table)),
                      _p(pad(q_kind)), _p(var_ptr), _p(pad(pos)), _p(pad(var_u)), _p(pad(var_type)), _p(snip_ptr), _p(snip_bytes), _p(bits_ptr), _p(bits), _p(count))
    out = []
    for q, (k, _, _, _) in enumerate(queries):
        sup = H._rows_of_bits(bits[int(bits_ptr[q]):int(bits_ptr[q + 1])], len(items[k][1])).tolist()
        assert len(sup) == count[q]
        out.append(sup)
    return out


def check_masks(T, items):
    """masks and prefix counts of every block against the strings"""
    r = 0
    for _, ra in items:
        for a, b, _ in ra.values():
            blk0 = int(T["blk_ptr"][r])
            bases = 0
            for blk in range((len(a) + 63) // 64):
                cols = range(blk * 64, min(len(a), blk * 64 + 64))
                nob = sum(1 << (j - blk * 64) for j in cols if a[j] == "-") | (M64 & ~((1 << len(cols)) - 1))
                diff = sum(1 << (j - blk * 64) for j in cols if a[j] != b[j])
                assert (int(T["nob"][blk0 + blk]), int(T["diff"][blk0 + blk]), int(T["pre"][blk0 + blk])) == (nob, diff, bases), (r, blk)
                bases += sum(1 for j in cols if a[j] != "-")
            assert int(T["out"][r, 3]) == bases
            r += 1


def check_case(L, items, queries):
    T = build(L, items)
    assert T["bad"] == 0
    check_masks(T, items)
    errors, sup = RC.expected(items, queries)
    assert np.array_equal(T["out"][:, :3].astype(np.int64), errors)
    got = support(L, T, items, queries)
    for q in range(len(queries)):
        assert got[q] == sup[q], (q, queries[q], got[q], sup[q])
    return sum(len(s) for s in sup)


def test_word_primitives(emul):
    rng = random.Random(5)
    masks = [0, M64, 1, 1 << 63, M64 >> 1, M64 & ~1, 0xAAAAAAAAAAAAAAAA] + [rng.getrandbits(64) for _ in range(40)] + [rng.getrandbits(64) | rng.getrandbits(64) for _ in range(10)]
    for m in masks:
        zeros = [j for j in range(64) if not (m >> j) & 1]
        for n in range(-1, 66):          # an empty word: every n selects bit n; a full word: nothing to select
            assert emul.rt_emul_select_zero(m, n) == (zeros[n] if 0 <= n < len(zeros) else 64), (hex(m), n)
        for n in range(0, 65):
            lead = next((j for j in range(n) if not (m >> j) & 1), n)
            trail = next((j for j in range(n) if not (m >> (n - 1 - j)) & 1), n)
            assert emul.rt_emul_lead_ones(m, n) == lead and emul.rt_emul_trail_ones(m, n) == trail, (hex(m), n)
    for w0, w1 in [(M64, 0), (0, M64), (1 << 63, 1)] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(20)]:
        wide = w0 | (w1 << 64)
        for sh in range(64):
            for n in (0, 1, 2, 63 - sh if sh < 63 else 1, 64 - sh, 64):          # 64 - sh: the window ends at bit 63
                assert emul.rt_emul_window(w0, w1, sh, n) == (wide >> sh) & ((1 << n) - 1), (sh, n)
    for b in (0, 1, 3):
        for lo in (0, 1, 63, 64, 65, 127, 128, 191, 192, 200, 255, 256, 300):
            for hi in (0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 257, 400):
                want = sum(1 << (j - 64 * b) for j in range(64 * b, 64 * b + 64) if lo <= j < hi)
                assert emul.rt_emul_range_mask(b, lo, hi) == want, (b, lo, hi)
    for pre in ([0], [0, 0, 0, 5], [0, 64, 128], [0, 3, 3, 3, 60, 61], [0, 0], [0, 10, 10, 10]):
        arr = np.asarray(pre, dtype=np.uint32)
        for i in range(0, pre[-1] + 3):
            assert emul.rt_emul_find_block(_p(arr), len(pre), i) == max(b for b in range(len(pre)) if pre[b] <= i), (pre, i)


def test_directed_shapes(emul):
    items, queries = RC.directed_case()
    assert check_case(emul, items, queries) > 100


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(emul, seed):
    items, queries = RC.random_case(seed)
    assert check_case(emul, items, queries) > 20


def test_rows_with_two_gaps_in_a_column_and_other_bytes(emul):
    """the error counts are read_errors_from_alignment for any rows over ACGT-, a column of two gaps included; any other byte is reported"""
    rng = random.Random(9)
    ra = {}
    for r in range(60):
        n = rng.choice([1, 2, 5, 63, 64, 65, 130, 200])
        ra["r%d" % r] = ("".join(rng.choice("ACGT---") for _ in range(n)), "".join(rng.choice("ACGT---") for _ in range(n)), ())
    ra["all_gaps"] = ("-" * 64, "A" * 64, ())
    ra["all_gaps_2"] = ("-" * 130, "-" * 130, ())
    T = build(emul, [(0, ra)])
    assert T["bad"] == 0
    check_masks(T, [(0, ra)])
    assert np.array_equal(T["out"][:, :3].astype(np.int64), RC.expected([(0, ra)], [])[0])
    assert build(emul, [(3, {"x": ("ACG", "ANG", ())})])["bad"] == 1 and build(emul, [(3, {"x": ("AcG", "ACG", ())})])["bad"] == 1


def test_reference_fixture(emul):
    """fixture g16: the reference's own supporters and error counts"""
    for items, queries, support_accs, errors in RC.g16_cases():
        T = build(emul, items)
        accs = [list(items[0][1]), list(items[1][1])]
        got = support(emul, T, items, queries)
        assert [accs[0][j] for j in got[0]] + [accs[1][j] for j in got[1]] == support_accs
        by_acc = dict(zip(accs[0] + accs[1], T["out"][:, :3].tolist()))
        assert [[a, by_acc[a]] for a, _ in errors] == errors
