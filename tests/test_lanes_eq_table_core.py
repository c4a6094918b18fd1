"""CPU: the match vectors of the pair-per-lane kernel's fast path from the lane's table of four masks (isocon_amd/csrc/ed_lanes_core.hpp
EqFromTable: what k_ed_lanes runs, with a plain array in place of LDS) against the ones built from the plane registers (EqFromPlanes, also
what the nine-argument call of lane_pair_distance still runs) and both distances against a textbook DP -- tests/emul/lanes_eq_table_emul.cpp,
a program of its own, built with g++ and a second time with -fsanitize=address,undefined.  Lengths m, n in {1, 31, 32, 33, 63, 64, 65, 95,
96, 97, 127, 128, 129, 257} with every threshold of {0, 1, 31, 32, 62, 63} that admits the pair, distances below, at and above the
threshold, texts of one base and of period 2 and 4 (every base at even and at odd columns), random pairs up to 3 kb; every Eq word of
every fast-path column must be equal, and nothing but the lane's own four records may be written."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "lanes_eq_table_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "ed_lanes_core.hpp")]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_table_form_equals_register_form_and_dp(build):
    exe = os.path.join(HERE, "emul", "_lanes_eq_table_emul" + ("" if build == "plain" else "_san"))
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    done = subprocess.run([exe] + ([] if build == "plain" else ["quick"]), capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout + done.stderr)[-3000:]
    f = done.stdout.split()
    pairs, fast_columns, end_blocks, within = (int(v) for v in f[1:5])
    assert f[0] == "ok", done.stdout
    # the grid alone is 4 500 pairs; the fast path ran (32 columns a block), also on windows that pass the pattern's end, and the pairs are
    # neither all within their threshold nor all beyond it
    assert pairs >= (5000 if build == "sanitized" else 8500), done.stdout
    assert fast_columns >= 32 * pairs and fast_columns % 32 == 0 and end_blocks > 1000, done.stdout
    assert pairs // 4 < within < pairs - pairs // 8, done.stdout
