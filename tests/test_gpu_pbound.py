"""GPU: Raghavan's bound of all tests of a round on the device (isocon_raghavan_bound: csrc/pbound.hpp k_pvalue_bound) through the C ABI and
the Python route -- every certified double against hypothesis_test_module._raghavan_from_sums as a 64-bit pattern on the four case lists of
tests/pbound_cases.py (shared with the CPU emulator test), batch sizes at the workgroup and grid edges, spare output slots, refusals, and
the switch behind do_statistical_tests_per_edge."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pbound_cases as BC  # noqa: E402
from isocon_amd import _lib  # noqa: E402
from isocon_amd import hypothesis_test_module as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["reference_sums", "random_in_domain", "planted"])
def test_in_domain_lists(name):
    """inside the domain: every test certified, every double the host's"""
    cases = getattr(BC, name)()
    before = dict(H.BOUND_STATS)
    bounds, certified = H._device_bounds(*BC.as_arrays(cases))
    assert BC.check(cases, bounds, certified, True) == len(cases)
    assert [H.BOUND_STATS[k] - before[k] for k in ("calls", "tests", "certified", "host_fallbacks")] == [1, len(cases), len(cases), 0]


def _resolved(m, y):
    """(m, y) as the one test of a round, through _resolve_bounds"""
    results, pending = {"e": ((), H._PendingBound(0), 0, 0)}, [(m, y)]
    H._resolve_bounds(results, pending)
    return results["e"][1]


def test_out_of_domain():
    """outside: nothing certified, 0.0 comes back, and the route returns or raises exactly what the host function does"""
    cases = BC.out_of_domain()
    bounds, certified = H._device_bounds(*BC.as_arrays(cases))
    assert BC.check(cases, bounds, certified, False) == 0
    for m, y in cases:
        want = BC.host(m, y)
        before = H.BOUND_STATS["host_fallbacks"]
        if want[0] == "raises":
            with pytest.raises(want[1]):
                _resolved(m, y)
        else:
            got = _resolved(m, y)
            assert type(got) is float and BC.bits(got) == want[1], (m, y)
        assert H.BOUND_STATS["host_fallbacks"] == before + 1
    assert type(_resolved(1.0, 0)) is float and _resolved(1.0, 0) == 1.0 and _resolved(2.5, 2.5) == 0.5          # (certified: no fallback)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_batch_sizes_and_spare_slots(n):
    """workgroup and grid edges; only the first n entries of the outputs are written"""
    pool = BC.random_in_domain() + BC.planted()
    cases = [pool[(7 * k) % len(pool)] for k in range(n)]
    m, y = BC.as_arrays(cases)
    m, y = np.append(m, [1.0, 2.0, 3.0]), np.append(y, [3.0, 2.0, 1.0])          # (beyond n: not to be read into the answers)
    bounds, certified = np.full(n + 3, 7.0), np.full(n + 3, 9, dtype=np.uint8)
    rc = _lib.lib().isocon_raghavan_bound(H._ptr(m, _lib.f64p), H._ptr(y, _lib.f64p), n, H._ptr(bounds, _lib.f64p), H._ptr(certified, _lib.u8p), None)
    assert rc == _lib.ISOCON_OK
    assert bounds[n:].tolist() == [7.0] * 3 and certified[n:].tolist() == [9] * 3
    assert BC.check(cases, bounds[:n], certified[:n], True) == n


def test_refused_arguments():
    L = _lib.lib()
    m, y, b, c = np.ones(4), np.ones(4), np.full(4, 7.0), np.full(4, 9, dtype=np.uint8)
    p = dict(m=H._ptr(m, _lib.f64p), y=H._ptr(y, _lib.f64p), b=H._ptr(b, _lib.f64p), c=H._ptr(c, _lib.u8p))
    for name in p:
        q = dict(p)
        q[name] = None
        assert L.isocon_raghavan_bound(q["m"], q["y"], 4, q["b"], q["c"], None) == _lib.ISOCON_E_ARG, name
    assert L.isocon_raghavan_bound(None, None, 0, None, None, None) == _lib.ISOCON_OK
    assert b.tolist() == [7.0] * 4 and c.tolist() == [9] * 4


class _Params(object):
    max_phred_q_trusted = 43


@pytest.mark.parametrize("with_qualities", [False, True], ids=["fasta", "fastq"])
def test_route(monkeypatch, with_qualities):
    """do_statistical_tests_per_edge on a small partition: the default route and ISOCON_DEBUG_VARIANT=stat_host_bound give equal dicts (p-values
    of the same type); one isocon_raghavan_bound call per round, no host evaluation, and no call under the switch"""
    C, partition, graph, X, ccs = BC.partition()
    out, calls = {}, {}
    for variant in (None, "stat_host_bound"):
        if variant:
            monkeypatch.setenv("ISOCON_DEBUG_VARIANT", variant)
        else:
            monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
        assert H.bounds_on_device_enabled() == (variant is None) and H.device_tables_enabled()
        H.clear_tables()
        before = dict(H.BOUND_STATS)
        out[variant] = H.do_statistical_tests_per_edge(graph, C, X if with_qualities else {}, partition, ccs if with_qualities else None, _Params())
        calls[variant] = {k: H.BOUND_STATS[k] - before[k] for k in ("calls", "tests", "certified", "host_fallbacks")}
        H.clear_tables()
    assert out[None] == out["stat_host_bound"]
    values = [v[0] for row in out[None].values() for v in row.values()]
    assert all(type(v) is float for v in values) and sum(v not in (0.0, 1.0) for v in values) >= 3
    n = calls[None]["tests"]
    assert n >= 3 and calls[None] == {"calls": 1, "tests": n, "certified": n, "host_fallbacks": 0}
    assert calls["stat_host_bound"] == {"calls": 0, "tests": 0, "certified": 0, "host_fallbacks": 0}


def test_route_sends_uncertified_sums_to_the_host(monkeypatch):
    """one edge whose sums are replaced by a pair on which the decimals overflow: the route evaluates it on the host and raises the host's exception"""
    import decimal
    C, partition, graph, X, ccs = BC.partition()
    monkeypatch.delenv("ISOCON_DEBUG_VARIANT", raising=False)
    bad = (900.6379341721139, 531940.3566810585)
    assert BC.host(*bad) == ("raises", decimal.Overflow)
    real, seen = H._raghavan_on_arrays, []

    def patched(prob, supporters, pending=None):
        at = real(prob, supporters, pending)
        seen.append(at)
        if pending is not None and len(pending) == 2:          # the second test of the round
            pending[-1] = bad
        return at

    monkeypatch.setattr(H, "_raghavan_on_arrays", patched)
    H.clear_tables()
    before = dict(H.BOUND_STATS)
    try:
        with pytest.raises(decimal.Overflow):
            H.do_statistical_tests_per_edge(graph, C, {}, partition, None, _Params())
    finally:
        H.clear_tables()
    assert len(seen) >= 3 and all(isinstance(at, H._PendingBound) for at in seen)
    assert H.BOUND_STATS["calls"] == before["calls"] + 1 and H.BOUND_STATS["host_fallbacks"] == before["host_fallbacks"] + 1
    assert H.BOUND_STATS["certified"] == before["certified"] + len(seen) - 1
