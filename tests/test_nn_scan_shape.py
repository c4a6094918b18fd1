"""CPU: the launch shapes of the table kernels (isocon_amd/csrc/nn_scan_shape.hpp) for every maxlen from 0 to 20 000, printed by a program of
its own (tests/emul/nn_scan_shape_main.cpp, built with g++ and a second time with -fsanitize=undefined,address), against a literal
restatement of the expressions the host code held in place before the header existed (commit 136a8f2; file:line of that commit)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "nn_scan_shape_main.cpp")
HDR = os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", "nn_scan_shape.hpp")
MAXLENS = range(0, 20001)
NN_RING = 96                    # nn.hpp:263
CU_LDS = 160 * 1024             # nn_main.inc:144
PAD = 40000


def lds_r(maxlen):              # nn_main.inc:143 (and inside lines 31, 37, 270, 274)
    return (4 * ((maxlen + 192 + 31) & ~31) + 160) * 4


def lds_h(maxlen):              # nn_main.inc:220
    return (4 * ((maxlen + 96 + 31) & ~31) + 96) * 4


def lds_w(maxlen, W):           # nn_wide.inc:12
    return (4 * ((maxlen + 192 * W + 31) & ~31) + 128 * W + 32) * 4


def ring(nw):                   # nn_main.inc:144 (ring8, ring16), nn_wide.inc:16
    return nw * NN_RING * 8 + 16


def refill_fits(maxlen):        # nn_main.inc:31, 37, 146, 270
    return lds_r(maxlen) + ring(16) <= CU_LDS


def ladder(maxlen, preferred, half):
    """(waves, dynamic LDS, limit raised) -- nn_main.inc:202-209 (64-row tables), 221-228 (32-row tables), 246-252 (unlisted: preferred = 4
    if `four`), 279-286 (2-set: preferred 8)"""
    lds = lds_h(maxlen) if half else lds_r(maxlen)
    if preferred == 4 and 3 * (lds + ring(8)) <= CU_LDS:
        return (4, lds, 0)
    if 3 * (lds + ring(8)) <= CU_LDS:
        return (8, lds, 0)
    return (16, lds, 1)          # hipFuncSetAttribute(... MaxDynamicSharedMemorySize ...) in front of the launch


def tile_scan(maxlen):
    """0: k_nn_scan_lds<8>, 1: k_nn_scan_lds<16>, 2: k_nn_scan_up<1> -- nn_main.inc:135, 253, 255, 258"""
    lds = (maxlen + 192) * 16
    return (0 if lds <= 53 * 1024 else 1 if lds <= 160 * 1024 else 2, lds)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def rows(request):
    exe = os.path.join(HERE, "emul", "_nn_scan_shape" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (SRC, HDR)):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wextra", "-o", exe, SRC])
    done = subprocess.run([exe, "--pad", str(PAD)], input="".join("%d\n" % m for m in MAXLENS), capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr[-2000:]
    out = [[int(x) for x in ln.split()] for ln in done.stdout.splitlines()]
    assert [r[0] for r in out] == list(MAXLENS) and all(len(r) == 44 for r in out)
    return out


def test_every_maxlen_gives_the_shapes_of_the_expressions_it_replaces(rows):
    for r in rows:
        m = r[0]
        assert r[1:5] == [ring(4), ring(8), ring(12), ring(16)], m
        assert r[5] == int(refill_fits(m)), m
        at = 6
        for preferred in (4, 8):
            for half in (0, 1):
                assert tuple(r[at:at + 3]) == ladder(m, preferred, half), (m, preferred, half)
                at += 3
        assert tuple(r[at:at + 2]) == tile_scan(m), m
        at += 2
        for W in range(2, 9):
            # nn_wide.inc:17 -- 12 waves for the 512-row form, 16 for the others (both printed for every W)
            assert r[at:at + 3] == [lds_w(m, W), int(lds_w(m, W) + ring(12) <= CU_LDS), int(lds_w(m, W) + ring(16) <= CU_LDS)], (m, W)
            at += 3
        assert r[at:] == [8, lds_r(m) + PAD, 1], m          # nn_main.inc:197-201 (nn_lds_pad)


def test_edges(rows):
    """where the shapes change, with NN_RING = 96 and 160 KB of LDS"""
    fits = [r[0] for r in rows if r[5]]
    assert fits == list(range(0, 9217))                                               # the refill kernel up to 9216
    for col, last in ((6, 2784), (9, 2880)):                                          # preferred 4: 64-row form, 32-row form
        three = [r[0] for r in rows if r[col] != 16]
        assert three == list(range(0, last + 1)) and all(r[col] == 4 and r[col + 6] == 8 for r in rows[:last + 1])
        assert all(r[col] == 16 and r[col + 6] == 16 and r[col + 2] == 1 for r in rows[last + 1:])
    kernel = [r[18] for r in rows]
    assert kernel[:3201] == [0] * 3201 and rows[3200][19] <= 53 * 1024 < rows[3201][19]     # k_nn_scan_lds<8> only below 3201
    assert kernel[3201:10049] == [1] * (10049 - 3201) and kernel[10049:] == [2] * (20001 - 10049)
    # without the refill kernel (9217 and up) the 16-wave k_nn_scan_lds runs up to 10048, the scalar-window kernel from 10049
    assert [m for m in MAXLENS if not refill_fits(m) and kernel[m] == 1] == list(range(9217, 10049))
    # one formula for every band: the 64 W-row form at W = 1 is the 64-row form
    assert all(lds_w(m, 1) == lds_r(m) for m in MAXLENS)
