"""CPU: the designed inputs of tests/hw_locations_wide_cases.py are what they claim under the restatement (hw_locations_cases.restated:
band above 512 diagonals, distance, number of ends, route), and the lane-level math of the two un-banded ends kernels of
isocon_hw_locations_wide -- csrc/hw_rows_core.hpp (one lane per pair) and mode ENDS of csrc/hw_full_core.hpp (one wavefront per pair), with
the un-banded START of an end -- gives the restatement's counts, ends and starts on them.  tests/emul/hw_rows_emul.cpp and
tests/emul/hw_full_ends_emul.cpp are programs of their own, built with g++ and a second time with -fsanitize=address,undefined, and run as
subprocesses."""
import os
import subprocess

import pytest

import hw_locations_wide_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc")
CORES = [os.path.join(CSRC, f) for f in ("hw_rows_core.hpp", "hw_full_core.hpp", "hw_core.hpp", "band_core.hpp")] + [os.path.join(HERE, "emul", "hw_wide_emul.hpp")]


# ---- the cases are what they claim ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", W.ALL_GROUPS)
def test_cases_are_what_they_claim(group):
    for c, (h, locs) in zip(W.cases(group), W.expected(group)):
        P, n = len(c.query), len(c.target)
        assert c.route == W.route_of(P, n, c.k), c.name
        if c.route in ("w1", "w2", "w4", "wave"):
            assert W.band(P, n, c.k) > 512, c.name
        if c.dist is not None:
            unbounded = W.restated(c.query, c.target, max(P, n))[0]
            assert unbounded == c.dist, (c.name, unbounded)
            assert h == (c.dist if c.dist <= c.k else -1), (c.name, h)
        if c.n_ends is not None:
            assert len(locs) == c.n_ends, (c.name, len(locs), locs[:8])
        assert [e for _, e in locs] == sorted({e for _, e in locs}), c.name


def test_groups_cover_the_issue():
    by = {g: {c.name: c for c in W.cases(g)} for g in W.ALL_GROUPS}
    # the routes the cases claim are those of the host's default switch and of the instances the lane kernel has
    host = open(os.path.join(CSRC, "hw_loc_wide_host.inc")).read()
    assert "kHwlRowsMax = %d;" % W.ROWS_MAX in host and all("k_hwl_rows<%d, FILL>" % w in host for w in (1, 2, 4))
    # every short query is wide against every target length, on the word count of its length; the long ones take the wavefront
    for P in W.SHORT_QUERIES:
        want = "w1" if P <= 64 else "w2" if P <= 128 else "w4"
        assert [by["edges"]["edges_q%d_t%d" % (P, n)].route for n in W.SHORT_TARGETS] == [want] * len(W.SHORT_TARGETS)
        assert [len(by["edges"]["edges_q%d_t%d" % (P, n)].target) for n in W.SHORT_TARGETS] == list(W.SHORT_TARGETS)
    for P in W.LONG_QUERIES:
        c = by["edges"]["edges_q%d" % P]
        assert c.route == "wave" and len(c.target) == P + 200 and c.k == P
    assert W.route_of(129, 700, 2, rows_max=64) == "wave" and W.route_of(64, 700, 2, rows_max=64) == "w1"
    exp = dict(zip((c.name for c in W.cases("copies")), W.expected("copies")))
    assert exp["copies_first_column"][1][0][0] == 0
    c = by["copies"]["copies_last_column"]
    assert exp[c.name][1][-1][1] == len(c.target) - 1
    assert [exp["copies_end%d" % e][1][0][1] % 64 for e in W.TEXT_LOAD_ENDS] == [31, 32, 33, 63, 64 % 64, 65 % 64]
    (s0, e0), (s1, e1) = exp["copies_overlap"][1]
    assert s1 <= e0          # the two copies overlap
    # every column an end: h = 20 on the banded START, h = 300 beyond it
    e20, e300 = W.expected("all")
    assert e20[0] == 20 and len(e20[1]) == 700 and e300[0] == 300 and len(e300[1]) == 310 and W.cases("all")[1].route == "wave"
    # thresholds: len(t) - len(q) == -k runs a kernel, one base less none
    assert by["thresholds"]["thr_short_by_k"].route == "wave" and by["thresholds"]["thr_short_by_k_plus_1"].route == "none"
    assert dict(zip((c.name for c in W.cases("thresholds")), W.expected("thresholds")))["thr_short_by_k"][0] == 300
    # lists: hits of 1 to 5 ends and misses in every list of more than a few pairs
    for size in W.LIST_SIZES:
        ends = [c.n_ends for c in W.cases("lanes") if c.name.startswith("lanes%d_" % size)]
        assert len(ends) == size and (size < 63 or set(ends) == {0, 1, 2, 3, 4, 5})
        assert all(c.route == "w1" for c in W.cases("lanes"))
    routes = [c.route for c in W.cases("mixed")]
    assert routes == ["narrow", "w1", "narrow", "w1", "w4", "none", "w4", "narrow"], routes
    seqs, q, t, k = W.random_list()
    kinds = {W.route_of(len(seqs[a]), len(seqs[b]), kk) for a, b, kk in zip(q, t, k)}
    assert kinds >= {"narrow", "w1", "w2", "w4", "wave"} and len(q) == 300


# ---- the emulators ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def ask(request):
    """ask(program, pairs, *args) -> [(h, counted, first, ((start, end), ...))] of the (query, target, k) in `pairs`"""
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    exes = {}
    for name in ("hw_rows_emul", "hw_full_ends_emul"):
        src = os.path.join(HERE, "emul", name + ".cpp")
        exe = os.path.join(HERE, "emul", "_" + name + ("" if request.param == "plain" else "_san"))
        if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + CORES):
            subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, src])
        exes[name] = exe

    def run(program, pairs, *args):
        text = "".join("%s %s %d\n" % (q or "-", t or "-", k) for q, t, k in pairs)
        done = subprocess.run([exes[program]] + [str(a) for a in args], input=text, capture_output=True, text=True)
        assert done.returncode == 0, (done.stdout[-1000:] + done.stderr)[-3000:]
        out = []
        for ln in done.stdout.splitlines():
            v = [int(x) for x in ln.split()]
            assert len(v) == 4 + 2 * v[3], ln[:200]
            out.append((v[0], v[1], v[2], tuple(zip(v[4::2], v[5::2]))))
        assert len(out) == len(pairs)
        return out
    return run


def check(got, pairs, names):
    for (h, counted, first, locs), (q, t, k), name in zip(got, pairs, names):
        eh, elocs = W.L.restated_cached(q, t, k)
        assert h == eh, (name, h, eh)
        # the count run and the fill run agree, and both with the restatement; the first end is the first location's
        assert counted == len(locs) == len(elocs), (name, counted, len(locs), len(elocs))
        assert first == (elocs[0][1] if elocs else -1), (name, first)
        assert locs == tuple(elocs), (name, locs[:4], elocs[:4])


def pairs_of(group, routes):
    cs = [c for c in W.cases(group) if c.route in routes]
    return [(c.query, c.target, c.k) for c in cs], [c.name for c in cs]


@pytest.mark.parametrize("group", W.ALL_GROUPS)
def test_rows_kernel_math(ask, group):
    pairs, names = pairs_of(group, ("w1", "w2", "w4", "narrow", "none"))
    check(ask("hw_rows_emul", pairs), pairs, names)


@pytest.mark.parametrize("words", (2, 4))
def test_rows_kernel_math_in_more_words_than_needed(ask, words):
    """a query in the low words of a wider instance: the last row's bit sits in a lower word than the instance's last"""
    pairs, names = pairs_of("copies", ("w1",))
    extra, more = pairs_of("edges", ("w1", "w2") if words == 4 else ("w1",))
    check(ask("hw_rows_emul", pairs + extra, words), pairs + extra, names + more)


@pytest.mark.parametrize("group", W.ALL_GROUPS)
def test_wavefront_mode_math(ask, group):
    """every case on the wavefront route, whatever its own is: 1 to 65 lanes, one and two passes"""
    cs = [c for c in W.cases(group) if group != "lanes" or c.name.startswith("lanes65_")]
    pairs, names = [(c.query, c.target, c.k) for c in cs], [c.name for c in cs]
    check(ask("hw_full_ends_emul", pairs), pairs, names)


def test_random_list_math(ask):
    seqs, q, t, k = W.random_list()
    pairs = [(seqs[a], seqs[b], kk) for a, b, kk in zip(q, t, k)]
    names = list(range(len(pairs)))
    short = [i for i, p in enumerate(pairs) if len(p[0]) <= 256]
    check(ask("hw_rows_emul", [pairs[i] for i in short]), [pairs[i] for i in short], short)
    check(ask("hw_full_ends_emul", pairs), pairs, names)
