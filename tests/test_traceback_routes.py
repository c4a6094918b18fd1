"""edlib_traceback (global mode) and edlib_traceback_allow_ends on whichever route the machine gives them -- the device with a GPU, the
host matrix without one -- against the reference's own function (fixture g21, made under the edlib stand-in) and the oracle."""
import pytest

from conftest import golden
from oracle import oracle as O


def test_allow_ends_against_the_reference_on_either_route():
    from isocon_amd import edlib_alignment_module as EAM
    from isocon_amd import end_invariant_functions as END
    g = golden("g21_traceback_allow_ends.json")
    before = dict(EAM.TRACEBACK_STATS)
    for c in g["cases"][::4]:
        got = END.edlib_traceback_allow_ends(c["x"], c["y"], mode="NW", task="path", k=c["k"], end_threshold=c["end_threshold"])
        assert got == (c["ed"], [tuple(l) for l in c["locations"]], c["cigar"]), c
    n = len(g["cases"][::4])
    assert sum(EAM.TRACEBACK_STATS.values()) - sum(before.values()) == n          # every call is counted on exactly one route
    with pytest.raises(NotImplementedError):
        END.edlib_traceback_allow_ends("ACGT", "ACGT", mode="HW")


def test_traceback_bound_on_either_route():
    from isocon_amd import edlib_alignment_module as EAM
    x, y = "ACGTACGTTGCA", "ACGACGTTTGCAA"
    ed, ops = O.nw_path(x, y)
    assert EAM.edlib_traceback(x, y, k=ed) == (ed, [(0, len(y) - 1)], "".join("%d%s" % o for o in ops))
    assert EAM.edlib_traceback(x, y, k=ed - 1) == (-1, [], None)
    assert EAM.edlib_traceback(x, y, k=-1)[0] == ed
