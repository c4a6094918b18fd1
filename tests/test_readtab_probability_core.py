"""CPU: the probability lane math of the device read tables (isocon_amd/csrc/readtab_core.hpp: rt_probability_step) driven by 64
emulated lanes in the shape of k_rt_probability (tests/emul/readtab_probability_emul.cpp: a program of its own that reads a case file and
writes a result file, built with g++ -O2 -ffp-contract=off and a second time with -fsanitize=undefined,address): every double against
hypothesis_test_module._ccs_probabilities_from_codes on the host tables' code bytes as 64-bit patterns, the status words, the quality
sweep against numpy's own p_error, and the reference's own probabilities of fixture g16.  Cases: tests/readtab_probability_cases.py,
shared with tests/test_gpu_readtab_probability.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readtab_probability_cases as PC  # noqa: E402
import readtab_quality_cases as QC  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

SRC = os.path.join(HERE, "emul", "readtab_probability_emul.cpp")
DEPS = [os.path.join(HERE, "emul", f) for f in ("readtab_quality_emul.cpp", "readtab_emul.cpp")] + \
       [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "readtab_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = os.path.join(HERE, "emul", "_readtab_probability_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + DEPS):
        subprocess.check_call(["g++"] + flags + ["-ffp-contract=off", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def run(exe, tmp_path, items, queries, ccs, ratios, max_phred_q_trusted, spare=0):
    """the emulated k_rt_probability over a table set: per query (float64 per row, status); spare: slots added to every query's range"""
    ref, read, row_ptr, first_row = H._pack_rows(items)
    rows = [(acc, v[1]) for _, ra in items for acc, v in ra.items()]
    recs = [ccs[acc] for acc, _ in rows]
    qual = np.asarray([q for r in recs for q in r.qual], dtype=np.uint8)
    qual_ptr = np.asarray(np.cumsum([0] + [len(r.qual) for r in recs]), dtype=np.uint64)
    rec_start = np.asarray([r.seq.index(row.replace("-", "")) for r, (_, row) in zip(recs, rows)], dtype=np.uint32)
    q_table, q_kind, var_ptr, var_pos, var_u, var_type, snip_ptr, snip_bytes, _ = H._pack_queries(QC.with_rows(items, queries))
    ref_len_of_var = np.repeat(np.asarray([items[k][0] for k in q_table.tolist()], dtype=np.int64), np.diff(var_ptr).astype(np.int64))
    pos = np.where(var_pos < 0, var_pos + ref_len_of_var, var_pos).astype(np.uint32)          # (what the host entry does before the launch)
    n_rows = [len(items[k][1]) for k, _, _, _ in queries]
    prob_ptr = np.asarray(np.cumsum([0] + [n + spare for n in n_rows]), dtype=np.uint64)
    arrays = [ref, read, row_ptr, first_row, qual, qual_ptr, rec_start, q_table, q_kind, var_ptr, pos, var_u, var_type, snip_ptr, snip_bytes,
              np.asarray(ratios, dtype=np.float64).reshape(len(queries), 3), H._p_of_quality(max_phred_q_trusted), prob_ptr]
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        for a in arrays:
            raw = np.ascontiguousarray(a).tobytes()
            f.write(np.uint64(len(raw)).tobytes() + raw)
    done = subprocess.run([exe, case, result], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    raw = open(result, "rb").read()
    n_prob = int(prob_ptr[-1])
    assert len(raw) == n_prob * 8 + len(queries) * 4
    prob, status = np.frombuffer(raw[:n_prob * 8], dtype=np.float64), np.frombuffer(raw[n_prob * 8:], dtype=np.uint32)
    for q, n in enumerate(n_rows):
        assert (prob[int(prob_ptr[q]) + n:int(prob_ptr[q + 1])].view(np.uint64) == 0).all()          # spare slots stay 0.0
    return [(prob[int(prob_ptr[q]):int(prob_ptr[q]) + n], int(status[q])) for q, n in enumerate(n_rows)]


def test_reference_fixture(emul, tmp_path):
    """fixture g16, all 70 cases in one table set: the reference's own 527 probabilities (repr-equal) and 33 non-informative reads"""
    items, queries, ccs, want = PC.g16_case()
    ratios = PC.table_ratios([H._ReadTable(ref_len, ra) for ref_len, ra in items], queries)
    got = run(emul, tmp_path, items, queries, ccs, ratios, 43)
    assert PC.check_g16(got, items, want) == (527, 33)
    assert PC.check(got, items, queries, ccs, ratios, 43)[0] == 0


@pytest.mark.parametrize("max_phred_q_trusted", [43, 30.5])
def test_directed_shapes(emul, tmp_path, max_phred_q_trusted):
    """tables of 0, 1, 63, 64, 65 and 130 rows, queries of 0, 1, 2 and many variants, every error code; a subnormal product and a product
    of 0.0 with the variant counts at which the host's own factor gets there; a read dropped at the second of three variants; the order of
    events across the 64-row passes and within a variant; spare slots"""
    items, queries, ccs, ratios, marks = PC.directed_case(max_phred_q_trusted)
    assert {len(ra) for _, ra in items} >= {0, 1, 63, 64, 65, 130, 71}
    assert {len(coords) for _, _, coords, _ in queries} >= {0, 1, 2, 3} and max(len(coords) for _, _, coords, _ in queries) > 50
    got = run(emul, tmp_path, items, queries, ccs, ratios, max_phred_q_trusted, spare=3)
    codes = QC.table_codes(items, queries, ccs)
    n_status, n_prob, n_dropped = PC.check(got, items, queries, ccs, ratios, max_phred_q_trusted, codes)
    assert n_status >= 8 and n_prob > 500 and n_dropped > 100, (n_status, n_prob, n_dropped)
    # the long products: the read of quality 93 is subnormal after k_sub variants and 0.0 after k_zero, on the host first
    q0, _ = marks["long"]
    want, _ = PC.host_answers(items, queries[q0:q0 + 4], ccs, ratios[q0:q0 + 4], max_phred_q_trusted, codes[q0:q0 + 4])
    for n in (0, 1):
        assert 0.0 < want[n][0][0] < PC.TINY and want[2 + n][0][0] == 0.0 and PC.TINY < want[2 + n][0][1] < 1.0
        assert got[q0 + n][0][0] == want[n][0][0] and got[q0 + 2 + n][0].tolist() == want[2 + n][0].tolist()
        with pytest.raises(AssertionError):
            H._ccs_probabilities_from_codes(2, queries[q0 + 2 + n][2], lambda v, *_: codes[q0 + 2 + n][v], ratios[q0], max_phred_q_trusted)
    # dropped at the second variant, both sequences shown at the third: -1.0 and no status
    q0, _ = marks["dropped"]
    for q in (q0, q0 + 1):
        assert codes[q][:, 0].tolist()[1:] == [QC.Q_NEITHER, QC.Q_BOTH] and codes[q][0, 0] <= 93
        assert got[q][1] == 0 and got[q][0][0] == -1.0 and got[q][0][1] > 0 and got[q][0][2] == -1.0
    # the order of events
    q0, _ = marks["order"]
    want = PC.status_order_case()[4]
    assert [got[q0 + n][1] for n in range(3)] == want
    assert codes[q0][0, 70] == QC.Q_INDEX and codes[q0][1, 3] == QC.Q_BOTH and sorted(codes[q0 + 2][0].tolist()) == [QC.Q_INDEX, QC.Q_BOTH]
    assert got[q0][0][70] == -2.0 and got[q0 + 1][0][3] == -2.0          # the rows that raised


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables(emul, tmp_path, seed):
    items, queries, ccs, ratios = PC.random_case(seed)
    got = run(emul, tmp_path, items, queries, ccs, ratios, 43)
    n_status, n_prob, n_dropped = PC.check(got, items, queries, ccs, ratios, 43)
    assert n_prob > 50 and n_dropped > 10, (n_status, n_prob, n_dropped)


@pytest.mark.parametrize("max_phred_q_trusted", [43, 20])
def test_quality_sweep(emul, tmp_path, max_phred_q_trusted):
    """every p_error of the 94 qualities x (S, I, D at u_v = 1; u_v = 2) x both kinds x nine ratio triples is numpy's, bit for bit"""
    items, queries, ccs, ratios, what = PC.sweep_case()
    got = run(emul, tmp_path, items, queries, ccs, ratios, max_phred_q_trusted)
    for (prob, status), want in zip(got, PC.sweep_expected(what, max_phred_q_trusted)):
        assert status == 0 and np.array_equal(prob.view(np.uint64), want.view(np.uint64))
    assert PC.check(got, items, queries, ccs, ratios, max_phred_q_trusted)[1] == 94 * len(queries)
