"""CPU: the routing of an explicit pair list through the distance stages (isocon_amd/csrc/ed_pairs_plan.hpp: shared side, sort, lanes / tiles
split, tile building and scatter-back, one-lane re-tiling of -2 lanes, escalation over 64 .. 512 rows, hand-over to the un-banded stage) with
the CPU emulators of tests/emul/band_emul.cpp and a textbook DP behind its backend, and the byte-range copy of the gathered upload
(gather_bytes in the same header) against a plain concatenation -- tests/emul/ed_pairs_plan_emul.cpp, a program of its own, built with g++ and
a second time with -fsanitize=address,undefined.  One shared sequence with 1, 15, 16, 17, 64, 65 and 129 partners; 64 partners with length
differences -63 .. +63 and k = d; planted distances 63/64, 127/128, 255/256, 511/512 with k = d - 1, d, d + 1 and unbounded in both argument
orders; empty sequences; a pair listed twice; a list whose second side is the shared one; min_group 0, 16 and unlimited.  Every pair must be
settled with the DP's answer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "emul", f) for f in ("ed_pairs_plan_emul.cpp", "band_emul.cpp")]
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("ed_pairs_plan.hpp", "band_core.hpp", "ed_lanes_core.hpp")]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_plan_and_gather_against_dp_and_concatenation(build):
    exe = os.path.join(HERE, "emul", "_ed_pairs_plan_emul" + ("" if build == "plain" else "_san"))
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in SRCS + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe] + SRCS)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout + done.stderr)[-3000:]
    got = {name: int(value) for name, value in (ln.split() for ln in done.stdout.splitlines())}
    assert got["ok"] == 1, done.stdout
    # every backend call received pairs under the default min_group: the lanes, both rounds of the tiles (the second only after a -2), every
    # band width and the un-banded stage
    for name in ("lanes", "tiles_round0", "tiles_round1", "minus2", "tiles_w1", "tiles_w2", "tiles_w4", "tiles_w8", "full"):
        assert got[name] > 0, (name, done.stdout)
    # ... the other two settings moved the groups: everything in tiles, everything in lanes; the exchanged list was tiled by its second side
    assert got["min_group0_tiles_w1"] == got["pairs"] == got["unlimited_lanes"] and got["swapped_tiles_round0"] > 0, done.stdout
    # the pairs are neither all within nor all beyond their thresholds
    assert got["within"] + got["beyond"] == got["pairs"] and got["within"] > got["pairs"] // 4 and got["beyond"] > got["pairs"] // 8, done.stdout
    assert got["gather_ranges"] > 1000 and got["gather_cuts"] == 400, done.stdout
