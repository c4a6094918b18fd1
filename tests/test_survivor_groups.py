"""CPU: where the survivor-list builder stages the kept pairs of a batch of 256 row positions and when a chunk leaves
(isocon_amd/csrc/nn_surv_core.hpp, called by k_nn_survivors) against a restatement of the loop it replaced -- 64 positions per step, one
per lane, the chunk check behind every step (tests/emul/survivor_groups_emul.cpp: a program of its own, built with g++ and a second
time with -fsanitize=undefined,address).  Random keep and class masks on rows of 0, 1, 3, 4, 63 .. 65, 255 .. 257 and 2 047 .. 2 305
positions, buffers that reach a chunk inside each of the four groups of a batch with every margin: the same chunks with the same
contents at the same places and the same remainders, in a buffer of exactly chunk + 64 words."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "survivor_groups_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f) for f in ("band_core.hpp", "nn_surv_core.hpp")]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_batches_stage_and_flush_as_steps_did(build):
    exe = os.path.join(HERE, "emul", "_survivor_groups" + ("" if build == "plain" else "_san"))
    flags = ["-O2"] if build == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout + done.stderr)[-2000:]
    f = done.stdout.split()
    cases, chunks, by_group = int(f[1]), int(f[2]), [int(v) for v in f[3:7]]
    # 269 row lengths x 5 keep rates x 4 class mixes x 2 (rep) + 4 groups x 64 margins x 3 mixes, for two chunk sizes
    assert f[0] == "ok" and cases == 2 * (269 * 5 * 4 * 2 + 4 * 64 * 3) and chunks > cases and min(by_group) > 1000, done.stdout
