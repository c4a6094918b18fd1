"""edlib_traceback_infix on whichever machine it runs: with a GPU the oracle's infix path, without one IsoconError -- it has no host
route, like the infix entry points; and edlib_traceback(mode="HW") keeps refusing."""
import pytest

from oracle import oracle as O


def test_infix_traceback_with_and_without_a_gpu():
    from isocon_amd import _lib
    from isocon_amd import edlib_alignment_module as EAM
    x, y = "GTACGTTGCAAC", "TTACGGTACGTGCAACGGA"
    before = dict(EAM.TRACEBACK_STATS)
    if _lib.load().isocon_device_count() > 0:
        e = O.hw_path(x, y, 3)
        assert e["editDistance"] == 1
        assert EAM.edlib_traceback_infix(x, y, k=3) == (e["editDistance"], e["locations"], e["cigar"])
        assert EAM.edlib_traceback_infix(x, y, k=0) == (-1, [], None)
    else:
        with pytest.raises(_lib.IsoconError):
            EAM.edlib_traceback_infix(x, y, k=3)
    assert EAM.TRACEBACK_STATS == before          # the two routes of edlib_traceback are not touched
    with pytest.raises(NotImplementedError):
        EAM.edlib_traceback(x, y, mode="HW")
