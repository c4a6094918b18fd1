"""CPU: what the host decides for the alignment path kernels without a device (isocon_amd/csrc/nwp_plan.hpp: classes, budgets and refusals,
the LDS bound, the order on the device, the slices of the reversed runs, the band waves, the cut of hits and waves into launches, the forward
offsets, and the same cut as isocon_hw_pairs_wide drives it) against a restatement in Python -- tests/emul/nwp_plan_emul.cpp, a program of its
own, built with g++ and a second time with -fsanitize=address,undefined.  The plan takes the distances as input, so a case is a list of
(len_q, len_t, ed[, start, cols]).  The program itself checks every plan it prints: ord a permutation, the un-banded positions first in list
order, the band positions by (class, columns, index), waves of 1 to 64 lanes of one class with the columns of their last and longest lane and
the unused slots at the tail, launches non-empty, of one class, within budget and cap, offsets and rev_off the running sums."""
import os
import random
import subprocess

import pytest

from test_nw_band_core import NOT_BANDED, band_class

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "nwp_plan_emul.cpp")
CORES = [os.path.join(os.path.dirname(HERE), "isocon_amd", "csrc", f)
         for f in ("nwp_plan.hpp", "nw_band_core.hpp", "nw_path_core.hpp", "hw_full_core.hpp", "hw_core.hpp", "ed_lanes_core.hpp", "band_core.hpp")]
E_HIP, E_UNSUPPORTED = -3, -6
GiB = 1 << 30
CAP = 1 << 20
MAX_LDS = 160 << 10


def test_status_codes():
    text = open(os.path.join(os.path.dirname(HERE), "include", "isocon_hip.h")).read()
    for name, value in (("ISOCON_E_HIP", E_HIP), ("ISOCON_E_UNSUPPORTED", E_UNSUPPORTED)):
        assert any(ln.split()[:3] == ["#define", name, str(value)] or ln.replace(",", " ").split()[:3] == [name, "=", str(value)] for ln in text.splitlines()), name


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def ask(request):
    """ask(text) -> the program's answer to the commands of `text`, as lines"""
    exe = os.path.join(HERE, "emul", "_nwp_plan_emul" + ("" if request.param == "plain" else "_san"))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [SRC] + CORES):
        subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, SRC])

    def run(text):
        done = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert done.returncode == 0, (done.stdout[-1000:] + done.stderr)[-3000:]
        return done.stdout.splitlines()
    return run


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def trace_units(m, ms):
    """hwf_trace_units (csrc/hw_full_core.hpp), as tests/test_gpu_ed_path.py restates it: 16-byte units of the un-banded store"""
    blocks = (m + 63) // 64
    last = (blocks + 63) // 64 - 1
    r32 = lambda u: (u + 31) & ~31
    lanes = blocks - 64 * last
    return r32((blocks + 1) // 2) + last * r32((ms + 63) * 64) + r32((ms + lanes - 1) * lanes)


def region_cols(cols):
    return (cols + 31) // 32 * 32


def greedy(units, budget, cap=CAP, new_launch=lambda i: False):
    """[(first, count, units)] and the offsets: an item joins the launch unless the bytes exceed the budget, the launch is full or new_launch"""
    launches, off, first, total = [], [], 0, 0
    for i, u in enumerate(units):
        if i > first and ((total + u) * 16 > budget or i - first >= cap or new_launch(i)):
            launches.append((first, i - first, total))
            first, total = i, 0
        off.append(total)
        total += u
    if units:
        launches.append((first, len(units) - first, total))
    return launches, off


def while_loop(units, budget):
    """the loop isocon_hw_pairs_wide had: consecutive hits while the sum fits, at most 2^20, offsets relative to the launch"""
    launches, off, a = [], [], 0
    while a < len(units):
        total, b = 0, a
        while b < len(units) and (total + units[b]) * 16 <= budget and b - a < CAP:
            off.append(total)
            total += units[b]
            b += 1
        launches.append((a, b - a, total))
        a = b
    return launches, off


def sizes(m, nt, cols, window):
    return "a query of %d bases against a target of %d bases" % (m, nt) + (" (window of %d columns)" % cols if window else "")


def expected(hits, budget=GiB, band_budget=GiB, unbanded=False, cap=CAP, pairs=None):
    """the plan of hits = [(len_q, len_t, ed[, start, cols])], or (status, text)"""
    window = len(hits[0]) == 5 if hits else False
    pairs = pairs or list(range(len(hits)))
    cls, cols, units, lds = [], [], [], 0
    for i, h in enumerate(hits):
        m, nt, ed = h[:3]
        nc = h[4] if window else nt
        if window and (h[3] < 0 or nc <= 0 or nc > nt - h[3]):
            return E_HIP, "internal status (window) for pair %d" % pairs[i]
        c = NOT_BANDED if unbanded or ed < abs(m - nc) else band_class(m, nc, ed)          # (a distance below the length difference: no such pair)
        if c:
            if region_cols(nc) * c * 16 > band_budget:
                return E_UNSUPPORTED, "the banded trace of %s needs %d bytes (budget %d)" % (sizes(m, nt, nc, window), region_cols(nc) * c * 16, band_budget)
        else:
            if trace_units(m, nc) * 16 > budget:
                return E_UNSUPPORTED, "the trace of %s needs %d bytes (budget %d)" % (sizes(m, nt, nc, window), trace_units(m, nc) * 16, budget)
            if m > 4096:
                lds = max(lds, (nc + 15) // 16 * 4)
        cls.append(c); cols.append(nc); units.append(0 if c else trace_units(m, nc))
    if lds > MAX_LDS:
        return E_UNSUPPORTED, "a query of more than 4096 bases against a target of more than %d bases is not supported" % (4 * MAX_LDS)
    n = len(hits)
    ord_ = [i for i in range(n) if not cls[i]] + sorted((i for i in range(n) if cls[i]), key=lambda i: (cls[i], cols[i], i))
    nu = cls.count(0)
    rev_off = [sum(2 * hits[i][2] + 1 for i in ord_[:p]) for p in range(n)]
    ulaunch, toff = greedy([units[i] for i in ord_[:nu]], budget, cap)
    waves, p = [], nu
    while p < n:
        W, e = cls[ord_[p]], p
        while e < n and e - p < 64 and cls[ord_[e]] == W:
            e += 1
        longest = region_cols(cols[ord_[e - 1]])
        if longest * W * (e - p) * 16 > band_budget:
            e = p + min(max(1, band_budget // (longest * W * 16)), e - p)
        longest = region_cols(cols[ord_[e - 1]])
        waves.append((W, longest, e - p, list(range(p, e))))
        p = e
    blaunch, woff = greedy([W * c * lanes for W, c, lanes, _ in waves], band_budget, cap, lambda w: waves[w][0] != waves[w - 1][0])
    return {"hits": n, "unbanded": nu, "w1": cls.count(1), "w2": cls.count(2), "w4": cls.count(4), "lds": lds, "rev_total": sum(2 * h[2] + 1 for h in hits),
            "cls": cls, "cols": cols, "units": units, "ord": ord_, "rev_off": rev_off, "ulaunch": ulaunch, "toff": toff,
            "wave": [(W, c, lanes, woff[w], pos) for w, (W, c, lanes, pos) in enumerate(waves)],
            "blaunch": [(a, cnt, waves[a][0], total) for a, cnt, total in blaunch],
            "stores": [max([t for _, _, t in ulaunch], default=0), sum(t for _, _, t in ulaunch), max([t for _, _, t in blaunch], default=0), sum(t for _, _, t in blaunch)]}


def plan_command(hits, budget=GiB, band_budget=GiB, unbanded=False, cap=CAP, pairs=None):
    window = len(hits[0]) == 5 if hits else False
    pairs = pairs or list(range(len(hits)))
    return "plan %d %d %d %d %d %d\n" % (budget, band_budget, unbanded, cap, window, len(hits)) + "".join("%d %s\n" % (p, " ".join(map(str, h))) for p, h in zip(pairs, hits))


def plans_of(lines):
    """the answers to plan commands: a dict like expected()'s, or (status, text)"""
    out, cur = [], None
    for ln in lines:
        f = ln.split()
        if f[0] == "refused":
            assert cur is None
            out.append((int(f[1]), ln.split(None, 2)[2]))
        elif f[0] == "hits":
            assert cur is None
            cur = {k: int(v) for k, v in zip(f[0::2], f[1::2])}
            cur.update(ulaunch=[], wave=[], blaunch=[])
        elif f[0] == "end":
            out.append(cur)
            cur = None
        elif f[0] in ("ulaunch", "blaunch"):
            cur[f[0]].append(tuple(int(x) for x in f[1:]))
        elif f[0] == "wave":
            cur["wave"].append(tuple(int(x) for x in f[1:5]) + ([int(x) for x in f[5:]],))
        else:
            cur[f[0]] = [int(x) for x in f[1:]]
    assert cur is None
    return out


def check(ask, cases):
    """cases: [(hits, keyword arguments)] -> the program's plans, each equal to the restated one"""
    got = plans_of(ask("".join(plan_command(h, **kw) for h, kw in cases)))
    assert len(got) == len(cases)
    for g, (h, kw) in zip(got, cases):
        assert g == expected(h, **kw), (h[:4], kw)
    return got


# ---- classes, order, waves ----------------------------------------------------------------------------------------------------------
CLASS_EDGES = ((0, 0), (0, 63), (0, 64), (0, 65), (5, 4), (-63, 63), (64, 64), (-127, 128), (128, 128), (0, 255), (0, 257), (256, 256))          # test_nw_band_core.py


def test_classes_at_their_edges(ask):
    hits = [(600 + d, 600, ed) for d, ed in CLASS_EDGES]
    banded, forced = check(ask, [(hits, {}), (hits, {"unbanded": True})])
    assert banded["cls"] == [1, 1, 2, 2, 0, 1, 2, 2, 4, 4, 0, 0] and (banded["w1"], banded["w2"], banded["w4"], banded["unbanded"]) == (3, 4, 2, 3)
    assert banded["ord"][:3] == [4, 10, 11] and [u > 0 for u in banded["units"]] == [c == 0 for c in banded["cls"]]
    assert [b[2] for b in banded["blaunch"]] == [1, 2, 4]          # a launch per class, whatever the budget
    assert forced["cls"] == [0] * 12 and forced["ord"] == list(range(12)) and not forced["wave"] and forced["ulaunch"] == [(0, 12, sum(forced["units"]))]
    assert forced["units"] == [trace_units(600 + d, 600) for d, _ in CLASS_EDGES]


def test_waves(ask):
    counts = (1, 63, 64, 65, 130)
    cases = [([(300 + (11 * i) % n, 300 + (11 * i) % n, 3) for i in range(n)], {}) for n in counts]          # class 1, distinct column counts, shuffled
    assert all(len(set(h[1] for h in hits)) == n for (hits, _), n in zip(cases, counts))
    got = check(ask, cases)
    assert [[w[2] for w in g["wave"]] for g in got] == [[1], [63], [64], [64, 1], [64, 64, 2]]
    assert all(g["w1"] == n and len(g["blaunch"]) == 1 and sorted(g["cols"]) == [g["cols"][i] for i in g["ord"]] for g, n in zip(got, counts))
    # classes 1, 2 and 4 behind three un-banded hits scattered through the list, over windows
    rng = random.Random(5)
    hits = []
    for i in range(150):
        ed = rng.choice([5, 40, 70, 100, 130, 200])
        cols = rng.randint(400, 700)
        hits.append((cols + rng.randint(-3, 3), 900, ed, rng.randint(0, 900 - cols), cols))
    for i in (0, 77, 149):
        hits[i] = (500, 900, 300, 10, 480)
    (g,) = check(ask, [(hits, {"pairs": [3 * i + 1 for i in range(150)]})])
    assert g["ord"][:3] == [0, 77, 149] and g["unbanded"] == 3 and min(g["w1"], g["w2"], g["w4"]) >= 20 and g["w1"] + g["w2"] + g["w4"] == 147
    assert sorted(set(w[0] for w in g["wave"])) == [1, 2, 4] and len(g["blaunch"]) == 3 and any(w[2] < 64 for w in g["wave"])
    assert check(ask, [([], {})])[0]["stores"] == [0, 0, 0, 0]


# ---- budgets ------------------------------------------------------------------------------------------------------------------------
def budget_hits(seed=13):
    rng = random.Random(seed)
    return [(m, m + rng.choice([-1, 0, 1]), 4) for m in (rng.randint(180, 220) for _ in range(9))]


def test_band_budget(ask):
    hits = budget_hits()
    cols32 = [region_cols(t) for _, t, _ in hits]
    region = max(cols32) * 9 * 16
    one, three, refused = check(ask, [(hits, {"band_budget": region}), (hits, {"band_budget": 3 * max(cols32) * 16}), (hits, {"band_budget": max(cols32) * 16 - 1})])
    assert one["w1"] == 9 and len(one["blaunch"]) == 1 and one["stores"][3] * 16 == region
    assert all(w[2] <= 3 for w in three["wave"]) and len(three["blaunch"]) == len(three["wave"]) >= 3 and three["stores"][3] * 16 <= region and three["w1"] == 9
    longest = max(hits, key=lambda h: (region_cols(h[1]), -hits.index(h)))
    assert refused == (E_UNSUPPORTED, "the banded trace of a query of %d bases against a target of %d bases needs %d bytes (budget %d)"
                       % (longest[0], longest[1], max(cols32) * 16, max(cols32) * 16 - 1))


def test_unbanded_budget(ask):
    hits = budget_hits()
    need = [trace_units(m, t) * 16 for m, t, _ in hits]
    assert max(need) < 2 * min(need)
    alone, threes, refused = check(ask, [(hits, {"budget": b, "unbanded": True}) for b in (max(need), 3 * max(need), max(need) - 1)])
    assert [l[1] for l in alone["ulaunch"]] == [1] * 9 and alone["stores"][0] * 16 == max(need) and alone["stores"][1] * 16 == sum(need)
    assert len(threes["ulaunch"]) >= 2 and all(3 <= l[1] <= 5 for l in threes["ulaunch"][:-1])          # (any three fit, and never six)
    big = need.index(max(need))
    assert refused == (E_UNSUPPORTED, "the trace of a query of %d bases against a target of %d bases needs %d bytes (budget %d)" % (hits[big][0], hits[big][1], max(need), max(need) - 1))


def test_launch_breaks(ask):
    far = [(300, 300 + i, 300) for i in range(8)]          # beyond 256 diagonals: un-banded
    near = [(300, 300 + 64 * i, 64 * i) for i in range(8)]          # a wave each (64 lanes at most; here: one hit per class change or not)
    many = [(300, 300 + i % 8, 8) for i in range(8 * 64)]          # eight full waves of class 1
    u, b, mixed = check(ask, [(far, {"cap": 3}), (many, {"cap": 3}), (near, {})])
    assert [l[:2] for l in u["ulaunch"]] == [(0, 3), (3, 3), (6, 2)]
    assert [l[:3] for l in b["blaunch"]] == [(0, 3, 1), (3, 3, 1), (6, 2, 1)] and len(b["wave"]) == 8
    # a class change starts a launch although the budget would hold everything
    assert [l[2] for l in mixed["blaunch"]] == sorted(set(c for c in mixed["cls"] if c)) and len(mixed["blaunch"]) >= 2 and mixed["stores"][3] * 16 < GiB


def test_lds_bound(ask):
    edge = 4 * MAX_LDS          # 655 360 columns: the boundary row fills the LDS limit
    small, none, at_limit, beyond = check(ask, [([(4097, 1000, 4000)], {"unbanded": True, "budget": 1 << 40}), ([(4096, 1000, 4000)], {"unbanded": True, "budget": 1 << 40}),
                                                ([(4097, edge, edge)], {"unbanded": True, "budget": 1 << 50}), ([(4097, edge + 1, edge)], {"unbanded": True, "budget": 1 << 50})])
    assert small["lds"] == (1000 + 15) // 16 * 4 and none["lds"] == 0 and at_limit["lds"] == MAX_LDS
    assert beyond == (E_UNSUPPORTED, "a query of more than 4096 bases against a target of more than 655360 bases is not supported")


def test_window_is_checked(ask):
    ok = [(100, 200, 3, 10, 100), (100, 200, 3, 0, 200)]
    for bad in ((100, 200, 3, -1, 100), (100, 200, 3, 5, 0), (100, 200, 3, 50, 151)):
        got = check(ask, [(ok + [bad], {"pairs": [4, 9, 17]}), ([bad] + ok, {"pairs": [4, 9, 17]})])
        assert got == [(E_HIP, "internal status (window) for pair 17"), (E_HIP, "internal status (window) for pair 4")]
    assert isinstance(check(ask, [(ok + [(100, 200, 3, 50, 150)], {})])[0], dict)


# ---- forward offsets, and the cut as isocon_hw_pairs_wide drives it -------------------------------------------------------------------
def test_forward_offsets(ask):
    rng = random.Random(3)
    n_pairs = 40
    hit_pairs = sorted(rng.sample(range(n_pairs), 17))
    runs = [rng.randint(1, 9) for _ in hit_pairs]
    ord_ = list(range(17))
    rng.shuffle(ord_)
    extra = [0 if p in hit_pairs else rng.choice([0, 1]) for p in range(n_pairs)]
    text = "offsets %d 17\n%s\n%s\n%s\n" % (n_pairs, "\n".join("%d %d" % x for x in zip(hit_pairs, runs)), " ".join(map(str, ord_)), " ".join(map(str, extra)))
    text += "offsets 5 0\n\n0 1 0 1 1\n"
    ptr, foff, ptr0, foff0 = [[int(x) for x in ln.split()[1:]] for ln in ask(text)]
    own = [runs[hit_pairs.index(p)] if p in hit_pairs else extra[p] for p in range(n_pairs)]
    assert ptr == [sum(own[:p]) for p in range(n_pairs + 1)] and 0 < sum(extra) < n_pairs - 17
    assert foff == [ptr[hit_pairs[h]] for h in ord_]
    assert ptr0 == [0, 0, 1, 1, 2, 3] and foff0 == []


def cuts_of(lines):
    out, cur = [], {"launch": []}
    for ln in lines:
        f = ln.split()
        if f[0] == "end":
            out.append(cur)
            cur = {"launch": []}
        elif f[0] == "launch":
            cur["launch"].append(tuple(int(x) for x in f[1:]))
        else:
            cur[f[0]] = [int(x) for x in f[1:]]
    return out


def test_cut_as_the_wide_infix_entry_drives_it(ask):
    """units like those of tests/test_gpu_hw_wide.py: queries of 300 to 337 rows ending 550 to 640 columns into their target"""
    rng = random.Random(77)
    units = [trace_units(rng.randint(300, 337), rng.randint(550, 640)) for _ in range(120)]
    need = [16 * u for u in units]
    assert max(need) < 2 * min(need)
    budgets = (max(need), 3 * max(need), 10 * min(need) + 5, GiB)
    got = cuts_of(ask("".join("cut %d 0 %d\n%s\n" % (b, len(units), " ".join(map(str, units))) for b in budgets) + "cut %d 3 8\n%s\n" % (GiB, " ".join(map(str, units[:8])))))
    for g, b in zip(got, budgets):
        launches, off = while_loop(units, b)
        assert (g["launch"], g["off"]) == (launches, off) == greedy(units, b)
        assert g["stores"] == [max(t for _, _, t in launches), sum(units)]
    # max < 2 min: the largest store alone in a budget of its size; three of it hold any three and never six
    assert [l[1] for l in got[0]["launch"]] == [1] * 120 and len(got[3]["launch"]) == 1 and all(3 <= l[1] <= 5 for l in got[1]["launch"][:-1])
    assert [l[:2] for l in got[4]["launch"]] == [(0, 3), (3, 3), (6, 2)]
