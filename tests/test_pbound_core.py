"""CPU: the lane math of Raghavan's bound on the device (isocon_amd/csrc/pbound_core.hpp: pb_eval) in the emulator of k_pvalue_bound
(tests/emul/pbound_emul.cpp: a program of its own that reads a case file and writes a result file, built with g++ -O2 and a second time
with -fsanitize=undefined,address): every certified double against hypothesis_test_module._raghavan_from_sums as a 64-bit pattern, every
case inside the domain certified, none outside, and the size of the error bound.  Cases: tests/pbound_cases.py, shared with
tests/test_gpu_pbound.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pbound_cases as BC  # noqa: E402

SRC = os.path.join(HERE, "emul", "pbound_emul.cpp")
DEPS = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "pbound_core.hpp")]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emul(request):
    exe = os.path.join(HERE, "emul", "_pbound_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + DEPS):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    return exe


def run(exe, tmp_path, cases):
    """(bounds, certified, err_total, distance to halfway in ulps of the result) of the emulated kernel"""
    m, y = BC.as_arrays(cases)
    case, result = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    np.stack([m, y], axis=1).tofile(case)
    done = subprocess.run([exe, case, result], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-3000:]
    raw, n = open(result, "rb").read(), len(cases)
    assert len(raw) == 25 * n
    return (np.frombuffer(raw[:8 * n], dtype=np.float64), np.frombuffer(raw[8 * n:9 * n], dtype=np.uint8), np.frombuffer(raw[9 * n:17 * n], dtype=np.float64),
            np.frombuffer(raw[17 * n:], dtype=np.float64))


def test_reference_sums(emul, tmp_path):
    """what fixture g16 hands to the bound, without and with base qualities: all certified, all the host's bits"""
    cases = BC.reference_sums()
    assert len(cases) == 210 and len(set(cases)) > 100          # (70 cases, three routes each)
    bounds, certified, err, _ = run(emul, tmp_path, cases)
    assert BC.check(cases, bounds, certified, True) == len(cases)
    assert err.max() <= 2.0 ** -100


def test_random_in_domain(emul, tmp_path):
    cases = BC.random_in_domain()
    assert len(cases) == 4000 and min(m for m, _ in cases) < 1e-55 and max(y for _, y in cases) > 5e4
    assert sum(abs(y / m - 1) <= 1e-6 for m, y in cases) > 1200
    bounds, certified, err, dist = run(emul, tmp_path, cases)
    assert BC.check(cases, bounds, certified, True) == len(cases)
    assert err.max() <= 2.0 ** -100          # (fails if precision is lost on the way: the bound is carried through every step)
    values = set(bounds.tolist())
    assert 1.0 in values and 0.0 in values and sum(0.0 < b < 1.0 for b in bounds.tolist()) > 1500
    assert (dist > 0).all()


def test_planted(emul, tmp_path):
    """the special cases, y one ulp either side of m, the steps to subnormal results, to the last subnormal and to 0.0, E ~ -800, d < 0"""
    cases = BC.planted()
    bounds, certified, err, _ = run(emul, tmp_path, cases)
    assert BC.check(cases, bounds, certified, True) == len(cases)
    assert err.max() <= 2.0 ** -100
    got = dict(zip([(float(m), float(y)) for m, y in cases], bounds.tolist()))
    assert got[(1.0, 0.0)] == 1.0 and got[(1.0, 1.0)] == 0.5 and got[(1e-30, 1e-30)] == 0.5
    kinds = {"normal": 0, "subnormal": 0, "zero": 0}
    for b in bounds.tolist():
        kinds["zero" if b == 0.0 else "subnormal" if b < BC.TINY else "normal"] += 1
    assert kinds["subnormal"] >= 4 and kinds["zero"] >= 2 and any(BC.TINY <= b < 2 * BC.TINY for b in bounds.tolist()) and BC.DENORM_MIN in bounds.tolist(), kinds


def test_out_of_domain(emul, tmp_path):
    """m = 0, negative, NaN, infinite and subnormal inputs, sums of 2^31 and more, and pairs on which the decimals overflow: not certified, 0.0"""
    cases = BC.out_of_domain()
    assert not any(BC.in_domain(m, y) for m, y in cases)
    assert any(BC.host(m, y)[0] == "raises" for m, y in cases)
    bounds, certified, _, _ = run(emul, tmp_path, cases)
    assert BC.check(cases, bounds, certified, False) == 0
