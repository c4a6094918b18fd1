"""GPU: the survivor-list builder with its keep test on four pairs per instruction (isocon_amd/csrc/nn_list.hpp k_nn_survivors<true>,
nn_surv_core.hpp surv_test4) against the same library with the test pair by pair (ISOCON_DEBUG_VARIANT=nn_surv_scalar) on the same
store: an identical graph (best, row_ptr, cols) and identical pairs_prefiltered, pairs_block_rejected, pairs_evaluated and
pairs_seed_known -- the counters that move when a pair is kept differently or a chunk is cut elsewhere."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("pairs_prefiltered", "pairs_block_rejected", "pairs_evaluated", "pairs_seed_known")


def _unique_by_length(seqs):
    return sorted(dict.fromkeys(seqs), key=len)


def _with_variant(variant, call):
    saved = os.environ.get("ISOCON_DEBUG_VARIANT")
    if variant:
        os.environ["ISOCON_DEBUG_VARIANT"] = variant
    elif saved is not None:
        del os.environ["ISOCON_DEBUG_VARIANT"]
    try:
        return call()
    finally:
        if saved is None:
            os.environ.pop("ISOCON_DEBUG_VARIANT", None)
        else:
            os.environ["ISOCON_DEBUG_VARIANT"] = saved


def _reads(n, length, isoforms, seed, rate=None):
    from isocon_amd import synth
    kw = {} if rate is None else {"profile": dict(synth.CCS_PROFILE, rate=rate)}
    return _unique_by_length(synth.make_reads(n, length, isoforms, seed=seed, **kw)[1])


def _both_forms_agree(st, variant="", **kw):
    packed = _with_variant(variant, lambda: st.nn_graph(**kw))
    single = _with_variant((variant + "," if variant else "") + "nn_surv_scalar", lambda: st.nn_graph(**kw))
    print(variant or "default", {k: packed[3][k] for k in COUNTERS}, "narrow", packed[3].get("pairs_narrow"))
    for a, b in zip(packed[:3], single[:3]):
        assert a.shape == b.shape and (a == b).all()
    assert {k: packed[3][k] for k in COUNTERS} == {k: single[3][k] for k in COUNTERS}
    return packed


# (a) all thresholds <= 31, short rows at both ends of the order; (b) nearest-neighbour distances 30 .. 60, both classes in one entry's
# buffer; (c) 50 .. 92, two thirds >= 64: thresholds at the cap and entries the 64-row phase hands on
STORES = {"a": (700, 300, 2, 77, None), "b": (400, 600, 3, 5, 0.05), "c": (400, 600, 3, 5, 0.08)}


@pytest.fixture(scope="module")
def stores():
    from isocon_amd.store import SeqStore
    open_stores = {}

    def get(name):
        if name not in open_stores:
            open_stores[name] = SeqStore(_reads(*STORES[name]))
        return open_stores[name]

    yield get
    for st in open_stores.values():
        st.close()


@pytest.mark.parametrize("name", sorted(STORES))
def test_same_lists_as_the_single_test(stores, name):
    g = _both_forms_agree(stores(name))
    assert g[3]["pairs_evaluated"] > 0 and (name == "c" or g[3]["pairs_prefiltered"] > 0)          # (c: thresholds at the cap, the bounds reject nothing)


def test_absent_directions(stores):
    """(d) A 2-set call (one in five a read, the others candidates) and a call with some converged entries: pairs with one direction or none."""
    st = stores("a")
    is_t = np.ones(st.n, np.uint8)
    is_t[::5] = 0
    assert is_t.sum() > 512          # (fewer candidates go through explicit tiles, without bounds and lists)
    g = _both_forms_agree(st, is_target=is_t)
    assert g[3]["pairs_prefiltered"] > 0
    conv = np.zeros(st.n, np.uint8)
    conv[1::3] = 1
    g = _both_forms_agree(st, is_converged=conv)
    assert g[3]["pairs_evaluated"] > 0


@pytest.mark.parametrize("narrow", [0, 1])
def test_other_class_modes(stores, narrow):
    """(e) nn_narrow=0: every pair in the 64-row class (the packed form without a class per pair); =1: the pairs above 31 leave the lists, a
    mode the library runs on the single test whatever the variant says -- the call still has to give the same lists."""
    _both_forms_agree(stores("b"), "nn_narrow=%d" % narrow)


def test_transposed_side_through_a_slot_map():
    """(f) Two ranks emulated in one process, as tests/test_gpu_survivor_scan.py test_sharded_map: on a rank's transposed rows a lane's four
    slots are consecutive entries only inside a block of the map, so the packed scan gathers its items where they cross one."""
    from isocon_amd import _lib
    from isocon_amd.dist import protocol_steps
    from isocon_amd.store import SeqStore, nn_finalize
    world = 2
    st = SeqStore(_reads(900, 300, 2, 78))
    try:
        n = st.n
        assert protocol_steps(0, world, n)[0][1][3] >= 4          # blocks of at least four entries: wide loads and gathers both occur

        def run():
            best = np.full(n, _lib.NN_INF, np.int32)
            hits_all, counters = [], dict.fromkeys(COUNTERS, 0)
            for k in range(len(protocol_steps(0, world, n))):
                parts = []
                for r in range(world):
                    phase, (qb, qe, qs, qk) = protocol_steps(r, world, n)[k]
                    b = best.copy()
                    if phase == 1:          # one pool for all ranks here: the rank's seed phase again, so that its matrix is the one in place
                        st.nn_partial(qb, qe, 0, np.full(n, _lib.NN_INF, np.int32), q_stride=qs, q_block=qk)
                    hits, stats = st.nn_partial(qb, qe, phase, b, q_stride=qs, q_block=qk)
                    for c in COUNTERS:
                        counters[c] += stats[c]
                    hits_all.append(hits)
                    parts.append(b)
                best = np.minimum.reduce(parts)
            hits = np.concatenate(hits_all)
            return nn_finalize(n, best, hits[(hits[:, 2] >= 0) & (hits[:, 2] == best[hits[:, 0]])]), counters

        packed, cp = _with_variant("", run)
        single, cs = _with_variant("nn_surv_scalar", run)
        print(cp)
        assert cp["pairs_prefiltered"] > 0 and cp == cs
        for a, b in zip(packed[:3], single[:3]):
            assert a.shape == b.shape and (a == b).all()
    finally:
        st.close()
