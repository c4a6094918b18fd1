"""CPU: the lane math of the edge variants (isocon_amd/csrc/edgevar_core.hpp) driven by 64 emulated lanes in the shape of k_ev_records /
k_ev_snippets (tests/emul/edgevar_emul.cpp: a program of its own, built with g++ and a second time with -fsanitize=undefined,address) on the
designed cases (tests/edgevar_cases.py) and on the 70 cases of the reference's fixture g16, whose values the reference itself made."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgevar_cases as EC  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

SRC = os.path.join(HERE, "emul", "edgevar_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "edgevar_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = os.path.join(HERE, "emul", "_edgevar_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def run(exe, edges):
    """edges: [(t, c, capacity, ops of (t, c), ops of (c, t))] -> [(bad, flipped, n_var, None if over the capacity else the records' rows)]"""
    seqs, index = [], {}
    for t, c, _, _, _ in edges:
        for x in (t, c):
            if x not in index:
                index[x] = len(seqs)
                seqs.append(x)
    lines = [str(len(seqs))] + seqs + [str(len(edges))]
    for t, c, cap, ops_tc, ops_ct in edges:
        lines.append(" ".join(str(v) for v in [index[t], index[c], cap, len(ops_tc)] + list(ops_tc) + [len(ops_ct)] + list(ops_ct)))
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    out = []
    for ln in done.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "E":
            out.append([int(f[1]), int(f[2]), int(f[3]), []])
        elif f[0] == "OVER":
            out[-1][3] = None
        else:
            out[-1][3].append(tuple(int(x) for x in f[1:7]) + (f[7], f[8], f[9], f[10], f[11]))
    assert len(out) == len(edges) and all(e[3] is None or len(e[3]) == e[2] for e in out)
    return [tuple(e) for e in out]


def edge_of(cs):
    ops_tc, ops_ct = EC.ops_of_case(cs)
    return (cs["t"], cs["c"], EC.capacity(ops_tc, ops_ct), ops_tc, ops_ct)


def as_tuple(rows):
    return H._file_variant_records([(r[0], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10]) for r in rows])


def test_designed_cases(emul):
    cases = EC.designed_cases()
    got = run(emul, [edge_of(cs) for cs in cases])
    seen = set()
    for cs, (bad, flipped, n_var, rows) in zip(cases, got):
        want_flipped, want_rows = EC.expected_records(cs)
        assert (bad, flipped, rows) == (0, int(want_flipped), want_rows), cs["name"]
        assert EC.same_tuple(as_tuple(rows), EC.expected_tuple(cs)), cs["name"]
        seen |= {r[6] for r in rows}
    assert seen == {"S", "I", "D"} and sum(e[1] for e in got) == 1 and max(e[2] for e in got) == 400


def test_reference_fixture(emul):
    """g16: the fixture's own variants, coordinates and snippets, dict order included"""
    cases = EC.g16_cases()
    got = run(emul, [edge_of(cs) for cs in cases])
    n_var = 0
    for cs, (bad, flipped, n, rows) in zip(cases, got):
        assert (bad, flipped) == (0, 0), cs["name"]
        assert EC.same_tuple(as_tuple(rows), cs["want"]), (cs["name"], as_tuple(rows), cs["want"])
        n_var += n
    assert len(cases) == 70 and n_var == sum(len(cs["want"][0]) for cs in cases) > 100


def test_refusals(emul):
    """ops that do not spell the two sequences, an unknown code, an empty op, no ops: bad and no record; a capacity one too small: the
    count and no record (the sanitized build would see a record written past the capacity)"""
    refused = EC.refused_ops()
    got = run(emul, [(t, c, 8, ops_tc, ops_ct) for _, t, c, ops_tc, ops_ct in refused])
    assert got == [(1, 0, 0, [])] * len(refused)
    exon = next(cs for cs in EC.designed_cases() if cs["name"] == "exon_400")
    t, c, cap, ops_tc, ops_ct = edge_of(exon)
    over, met = run(emul, [(t, c, cap - 1, ops_tc, ops_ct), (t, c, cap, ops_tc, ops_ct)])
    assert over == (0, 0, 400, None) and met[:3] == (0, 0, 400) and len(met[3]) == 400
