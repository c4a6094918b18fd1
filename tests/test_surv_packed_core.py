"""CPU: the keep test of the survivor-list builder on a lane's four pairs at once (isocon_amd/csrc/nn_surv_core.hpp surv_test4, surv_narrow4:
a byte per pair, guard-bit compares) against the test of one pair (surv_test, the definition and the kernel's other form) -- every output
bit of every case (tests/emul/surv_packed_emul.cpp: a program of its own, built with g++ and a second time with
-fsanitize=address,undefined).  The plain build sweeps bound 0 .. 255 x length difference 0 .. 127 x a 0 .. 65 x b 0 .. 65 (1.4 10^8 single
tests, every (bound, difference, b) and every a in each of the four byte positions), the caps 0 / 31 / 63 with every role combination
and every count of positions inside the row, and whole rows through the staging arithmetic: the same writes, chunks and counts from
byte masks as from single tests.  The sanitized build runs the same program with every 15th bound and every 7th row length."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "surv_packed_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "nn_surv_core.hpp")]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_four_pairs_at_once_equal_single_tests(build):
    exe = os.path.join(HERE, "emul", "_surv_packed" + ("" if build == "plain" else "_san"))
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    done = subprocess.run([exe] + ([] if build == "plain" else ["quick"]), capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout + done.stderr)[-3000:]
    f = done.stdout.split()
    tuples, caps, rows, chunks, kept = (int(v) for v in f[1:6])
    bounds = 256 if build == "plain" else 18
    lengths = 13 + (259 if build == "plain" else 37)
    assert f[0] == "ok" and tuples == bounds * 128 * 66 * 66 and caps == 3 * 2 * 3 * 5 * 16 * 65 * 24, done.stdout
    # two chunk sizes x row lengths x 4 keep mixes x 2 sides; chunks left the buffer and pairs were kept
    assert rows == 2 * lengths * 4 * 2 and chunks > rows / 8 and kept > 100 * rows, done.stdout
