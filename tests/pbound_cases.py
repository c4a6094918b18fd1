"""The cases of Raghavan's bound on the device (isocon_raghavan_bound: csrc/pbound_core.hpp), shared by tests/test_pbound_core.py (the CPU
emulator) and tests/test_gpu_pbound.py: lists of (m_sum, y_sum), each answer compared with hypothesis_test_module._raghavan_from_sums as a
64-bit pattern.  The first three lists lie inside the certified domain and must come back certified; the fourth lies outside and must not."""
import math
import os
import random
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edgevar_cases as EC  # noqa: E402
import readtab_cases as RC  # noqa: E402
import readtab_quality_cases as QC  # noqa: E402
from isocon_amd import ccs_info  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

TINY = float(np.finfo(np.float64).tiny)          # 2^-1022
DENORM_MIN = 5e-324                              # 2^-1074


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def host(m, y):
    """what _raghavan_from_sums does with (m, y): ("bits", the double's 64 bits) or ("raises", the exception's type)"""
    try:
        return "bits", bits(H._raghavan_from_sums(m, y))
    except Exception as e:          # decimal.Overflow, DivisionByZero, InvalidOperation, ValueError ...
        return "raises", type(e)


def in_domain(m, y):
    """the certified domain with a little room to its two decimal limits (the lanes compare against floor(9e5 ln 10)) and to the smallest
    ratio (the lanes compare the doubles' exponents: e_y - e_m >= -300)"""
    if not (0.0 < m < 2.0 ** 31 and 0.0 < y < 2.0 ** 31 and m >= TINY and y >= TINY):
        return False
    if y / m < 2.0 ** -299:
        return False
    return y * abs(math.log10(y / m)) <= 8.99e5 and abs(y - m) * math.log10(math.e) <= 8.99e5


_REFERENCE = None


def reference_sums():
    """the (m_sum, y_sum) that the 70 cases of fixture g16 hand to _raghavan_from_sums on the host tables, without base qualities (FASTA),
    with the fixture's qualities and with those put through fix_quality_values (FASTQ); y_sum is the int 0 where no read supports"""
    global _REFERENCE
    if _REFERENCE is not None:
        return _REFERENCE
    seen = []
    real = H._raghavan_from_sums

    def record(m_sum, y_sum):
        seen.append((m_sum, y_sum))
        return real(m_sum, y_sum)

    H._raghavan_from_sums = record
    try:
        for g, (items, _, recs, _, _) in zip(EC.g16_cases(), QC.g16_quality_cases()):
            (len_c, rc), (len_t, rt) = items
            assert len_c == len(g["c"]) and len_t == len(g["t"])
            fixed = {a: ccs_info.CCS(a, r.seq, ccs_info.fix_quality_values(r.seq, list(r.qual)), "NA") for a, r in recs.items()}
            for ccs in (None, recs, fixed):
                try:
                    H._test_on_tables(g["t"], g["c"], g["tc"], g["ct"], H._ReadTable(len_c, rc), H._ReadTable(len_t, rt), ccs, 43)
                except (AssertionError, IndexError, SystemExit):
                    pass
    finally:
        H._raghavan_from_sums = real
    _REFERENCE = seen
    return seen


def random_in_domain(seed=20):
    """4 000 seeded pairs: m = 10^U(-8, 3), y / m = 10^U(-3, 3), 30 % with |y / m - 1| <= 1e-6, 10 % with y = nextafter(m, +-); a block with
    m down to 1e-60 (products of many variant probabilities); a block with y up to 1e5.  Pairs outside the domain are drawn again."""
    rng = random.Random(seed)

    def pair(m_lo, m_hi):
        m = 10 ** rng.uniform(m_lo, m_hi)
        r = rng.random()
        if r < 0.1:
            return m, math.nextafter(m, math.inf if rng.random() < 0.5 else 0.0)
        if r < 0.4:
            return m, m * (1 + rng.uniform(-1e-6, 1e-6))
        return m, m * 10 ** rng.uniform(-3, 3)

    def large():
        y = 10 ** rng.uniform(2, 5)
        return y / 10 ** rng.uniform(-0.5, 3), y

    out = []
    for n, draw in ((3000, lambda: pair(-8, 3)), (500, lambda: pair(-60, -8)), (500, large)):
        got = 0
        while got < n:
            m, y = draw()
            if in_domain(m, y):
                out.append((m, y))
                got += 1
    return out


def _step(pred):
    """the smallest double y > 1 with pred(result of (1.0, y)): bisection on the host over the doubles' order"""
    lo, hi = bits(100.0), bits(300.0)
    assert not pred(H._raghavan_from_sums(1.0, 100.0)) and pred(H._raghavan_from_sums(1.0, 300.0))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(H._raghavan_from_sums(1.0, struct.unpack("<d", struct.pack("<Q", mid))[0])):
            hi = mid
        else:
            lo = mid
    return struct.unpack("<d", struct.pack("<Q", hi))[0]


_PLANTED = None


def planted():
    global _PLANTED
    if _PLANTED is not None:
        return _PLANTED
    out = [(1.0, 0), (1.0, 0.0), (3.5e-12, 0), (1.0, 1.0), (0.37, 0.37), (1e-30, 1e-30)]
    for m in (1e-30, 1.0, 1e4):
        out += [(m, math.nextafter(m, 0.0)), (m, math.nextafter(m, math.inf))]
    steps = []
    for pred in (lambda f: f < TINY, lambda f: f <= DENORM_MIN, lambda f: f == 0.0):          # E = ln 2^-1022, ln 2^-1074 (nearly), ln 2^-1075
        y = _step(pred)
        steps.append(y)
        out += [(1.0, math.nextafter(y, 0.0)), (1.0, y), (1.0, math.nextafter(y, math.inf))]
    assert 170.8 < steps[0] < 170.9 and 177.7 < steps[1] < steps[2] < 178.0, steps
    y = _step(lambda f: f == 0.0)
    while 1.0 - y + y * math.log(y) < 800.0:          # E ~ -800
        y += 0.25
    out.append((1.0, y))
    out += [(1.0, 10.0 ** -k) for k in range(1, 7)] + [(250.0, 250e-6), (3e-9, 3e-15)]          # d < 0 down to y / m = 1e-6
    # ... and the small-ratio side of the domain, where the host's 1 + d keeps ever fewer digits of y / m: down to y / m = 2^-299
    out += [(1.0, 1e-20), (37.5, 37.5e-35), (1.0, 1e-50), (2.5e-3, 2.5e-73), (1.0, 1e-90), (1000.0, 1e-87), (1e5, 3e-85), (1.0, 2.0 ** -299), (1.5, 2.0 ** -298),
            (1.9999999, 2.0 ** -298), (3e-200, 3e-290), (2.0e6, 2.0e6 * 2.0 ** -290)]
    assert all(in_domain(m, y) or y == 0 for m, y in out)
    _PLANTED = out
    return out


def out_of_domain():
    nan, inf, sub = float("nan"), float("inf"), 1e-310
    return [(0.0, 1.0), (0.0, 0.0), (0.0, 0), (-0.0, 1.0), (-1.0, 1.0), (-1.0, 0.0), (1.0, -1.0), (1.0, -0.0), (nan, 1.0), (1.0, nan), (nan, 0.0), (inf, 1.0), (1.0, inf),
            (inf, inf), (-inf, 1.0), (sub, 1.0), (1.0, sub), (sub, sub), (sub, 0.0), (5e-324, 5e-324), (1.0, 2.0 ** 31), (2.0 ** 31, 1.0), (2.0 ** 31, 2.0 ** 31),
            (3.0, 1e300), (1e300, 3.0), (900.6379341721139, 531940.3566810585), (992.5322917595573, 502727.4726648845), (1e-200, 5e5), (2.0 ** 30, 1e-300),
            # y / m so small that the host's d = y / m - 1 keeps no digit of it (it raises: 0 ** 0), or below the lanes' limit of 2^-301
            (1.0, 1e-150), (1.0, 1e-101), (1.0, 1e-300), (5.0, 2.3e-308), (1000.0, 1e-120), (1e-100, 1e-250), (1.0, 1e-100), (1.0, 1e-95), (1.0, 2.0 ** -302),
            (1.999, 2.0 ** -301), (1e-5, 1e-99)]


def as_arrays(cases):
    return (np.asarray([float(m) for m, _ in cases], dtype=np.float64), np.asarray([float(y) for _, y in cases], dtype=np.float64))


def check(cases, bounds, certified, must_certify):
    """every certified answer has the host's 64 bits, every other answer is 0.0 and -- where must_certify -- there is none; returns the
    number of certified answers"""
    bounds = np.asarray(bounds, dtype=np.float64).view(np.uint64).tolist()
    certified = np.asarray(certified).astype(bool).tolist()
    assert len(bounds) == len(certified) == len(cases)
    for (m, y), b, c in zip(cases, bounds, certified):
        if c:
            assert host(m, y) == ("bits", b), (m, y, host(m, y), b)
        else:
            assert not must_certify, (m, y)
            assert b == 0, (m, y, b)
    return sum(certified)


def partition():
    """candidates, their reads (stored alignments), the graph c -> t and the reads' records from the first trials of the generator: the
    edges of the route test of tests/test_gpu_readtab_probability.py"""
    rng = random.Random(3)
    C, part, graph, X = {}, {}, {}, {}
    for n, (t, c, _, _, reads_c, reads_t) in enumerate(RC.stat_trials()[:8]):
        C["t%d" % n], C["c%d" % n] = t, c
        part["c%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_c.items()}
        part["t%d" % n] = {"%d_%s" % (n, a): v for a, v in reads_t.items()}
        graph["c%d" % n] = {"t%d" % n: 1}
    for ra in part.values():
        for acc, v in ra.items():
            X[acc] = v[1].replace("-", "")
    ccs = {acc: QC.record(rng, acc, x, prefix="", suffix="") for acc, x in X.items()}
    return C, part, graph, X, ccs
