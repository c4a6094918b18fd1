"""GPU drop-in for /root/reference/modules/edlib_alignment_module.py (same names, arguments, return shapes).

All distances come from isocon_ed_pairs (include/isocon_hip.h); `nr_cores` is accepted and ignored (the reference
forks a Pool per call, EAM:28-41 -- here one batched launch replaces it).
"""
from __future__ import annotations

import numpy as np

from . import _lib, perf_log
from .store import SeqStore, store_for_pairs


def _intern(pairs):
    """[(x, y), ...] -> (unique sequence list, a ids, b ids)."""
    index, seqs = {}, []
    a = np.empty(len(pairs), dtype=np.uint32)
    b = np.empty(len(pairs), dtype=np.uint32)
    for p, (x, y) in enumerate(pairs):
        ia = index.get(x)
        if ia is None:
            ia = index[x] = len(seqs)
            seqs.append(x)
        ib = index.get(y)
        if ib is None:
            ib = index[y] = len(seqs)
            seqs.append(y)
        a[p], b[p] = ia, ib
    return seqs, a, b


def _distances(pairs):
    if not pairs:
        return np.zeros(0, dtype=np.int32)
    with perf_log.call("edlib_alignment_module.distances", pairs=len(pairs)) as rec:
        st, a, b, owned = store_for_pairs(pairs)
        try:
            ed, ms = st.ed_pairs(a, b, None, return_ms=True)
            rec.add(kernel_ms=ms)
        finally:
            if owned:
                st.close()
    assert (ed >= 0).all()  # EAM:113
    return ed


def edlib_align_sequences(matches, nr_cores=1):
    """EAM:10-49.  {s1: iterable(s2)} -> {s1: {s2: ed}} keyed by the sequences; keys without members are absent."""
    H = _lib.pyhelp()
    if H is not None and hasattr(H, "pairs_of") and type(matches) is dict and matches:
        # on the store the NN graph remembered (the pipeline's case, isocon_get_candidates.py:129-130,38): pairs, ids and the dict of dicts in C
        # without a tuple per pair (cpy/_pyhelp.c): 19 -> 10 ms for the 49 990 partition pairs of C3
        from . import store as _store
        st, index = _store._RECENT["store"], _store._RECENT["index"]
        if st is not None and index is not None and getattr(st, "_h", None):
            n = sum(len(v) for v in matches.values())
            a = np.empty(max(n, 1), dtype=np.uint32)
            b = np.empty(max(n, 1), dtype=np.uint32)
            rows = H.pairs_of(matches, index.mapping(), a.ctypes.data, b.ctypes.data, n)
            if rows is not None:
                outer, counts, inner = rows
                if not inner:
                    return {}
                with perf_log.call("edlib_alignment_module.distances", pairs=len(inner)) as rec:
                    ed, ms = st.ed_pairs(a[:len(inner)], b[:len(inner)], None, return_ms=True)
                    rec.add(kernel_ms=ms)
                assert (ed >= 0).all()  # EAM:113
                ed = np.ascontiguousarray(ed, dtype=np.int32)
                return H.distance_rows(outer, counts, inner, ed.ctypes.data)
    if H is not None and hasattr(H, "distance_dict") and type(matches) is dict and matches and \
            all(type(v) in (set, frozenset, list, tuple, dict) for v in matches.values()) and len(set(type(v) is dict for v in matches.values())) == 1:
        # the pair list, the ids and the dict of dicts in C (cpy/_pyhelp.c): 19 -> 6 ms for the 49 990 partition pairs of C3
        pairs = H.flatten_pairs(matches)[0]
        ed = np.ascontiguousarray(_distances(pairs), dtype=np.int32)
        return H.distance_dict(pairs, ed.ctypes.data)
    pairs = [(s1, s2) for s1 in matches for s2 in matches[s1]]
    ed = _distances(pairs)
    exact_edit_distances = {}
    for (s1, s2), d in zip(pairs, ed):
        exact_edit_distances.setdefault(s1, {})[s2] = int(d)
    return exact_edit_distances


def edlib_align_sequences_keeping_accession(matches, nr_cores=1):
    """EAM:51-99.  {acc1: {acc2: (s1, s2)}} -> {acc1: {acc2: (s1, s2, ed)}}."""
    keys = [(a1, a2) for a1 in matches for a2 in matches[a1]]
    pairs = [(matches[a1][a2][0], matches[a1][a2][1]) for a1, a2 in keys]
    ed = _distances(pairs)
    exact_matches = {}
    for (a1, a2), (s1, s2), d in zip(keys, pairs, ed):
        exact_matches.setdefault(a1, {})[a2] = (s1, s2, int(d))
    return exact_matches


def edlib_alignment(x, y, i, j, x_acc="", y_acc=""):
    """EAM:107-128 (single pair)."""
    ed = int(_distances([(x, y)])[0])
    if x_acc == y_acc == "":
        return (x, y, ed)
    return (x_acc, y_acc, (x, y, ed))


def edlib_alignment_helper(arguments):
    """EAM:103-105."""
    args, kwargs = arguments
    return edlib_alignment(*args, **kwargs)


# which route edlib_traceback took, per call: the device (isocon_ed_path_pairs) or the host (functions.nw_path_cigar)
TRACEBACK_STATS = {"device": 0, "host": 0}
# the calls of edlib_traceback_infix (isocon_hw_path_pairs; it has the device route alone).  A dict of its own: TRACEBACK_STATS holds
# exactly the two routes of edlib_traceback, and its callers compare it whole
TRACEBACK_INFIX_STATS = {"device": 0}
# the calls of edlib_traceback_infix_all (isocon_hw_locations + isocon_hw_path_pairs; the device route alone)
TRACEBACK_INFIX_ALL_STATS = {"device": 0}
# the calls of edlib_traceback_prefix (isocon_shw_locations + isocon_shw_path_pairs; the device route alone)
TRACEBACK_PREFIX_STATS = {"device": 0}


def _cigar_of_steps(steps):
    cigar, i = [], 0
    while i < len(steps):
        j = i
        while j < len(steps) and steps[j] == steps[i]:
            j += 1
        cigar.append("%d%s" % (j - i, steps[i]))
        i = j
    return "".join(cigar)


def edlib_traceback(x, y, mode="NW", task="path", k=1):
    """EAM:130-135: (editDistance, locations, cigar) of edlib.align(x, y, mode="NW", task="path", k=k).  Its only caller
    (isocon_statistical_test.get_nearest_neighbor_graph, :63-104) is never called in v0.3.3.  Distance
    and path come from the GPU (SeqStore.ed_path_pairs: the k-bounded distance first, the path of a hit from the trace
    kernels: banded on the diagonals within the distance where those are at most 256, un-banded -- with a trace of about
    len(x) * len(y) / 4 bytes that must fit 1 GiB -- beyond), with the tie rule used everywhere else (from the end: I, then D, then the diagonal; "parity unpinned");
    above k edlib reports (-1, [], None).  Two cases stay on the host (functions.nw_path_cigar, a full matrix in Python:
    short sequences only): a pair that holds more than four distinct symbols (the path kernels run on the 2-bit planes;
    its distance still comes from the GPU), and a machine without a GPU.  TRACEBACK_STATS counts the calls per route.
    HW mode lives in end_invariant_functions.edlib_traceback."""
    if mode != "NW" or task != "path":
        raise NotImplementedError("edlib_alignment_module.edlib_traceback: only mode='NW', task='path' (EAM:130-135)")
    kk = None if k is None or k < 0 else int(k)
    have_gpu = _lib.load().isocon_device_count() > 0
    if have_gpu and len(set(x) | set(y)) <= 4:
        st = SeqStore([x, y])
        try:
            ed, ops, _ = st.ed_path_pairs([0], [1], None if kk is None else [kk])
        finally:
            st.close()
        TRACEBACK_STATS["device"] += 1
        if ed[0] < 0:
            return -1, [], None
        return int(ed[0]), [(0, len(y) - 1)], "".join("%d%s" % (o >> 4, "=XID"[o & 15]) for o in ops.tolist())
    from .functions import nw_path_cigar
    TRACEBACK_STATS["host"] += 1
    if have_gpu:
        st = SeqStore([x, y])
        try:
            ed = int(st.ed_pairs([0], [1], None if kk is None else [kk])[0])
        finally:
            st.close()
        if ed < 0:
            return -1, [], None
        steps = nw_path_cigar(x, y)
    else:
        steps = nw_path_cigar(x, y)
        ed = sum(1 for c in steps if c != "=")
        if kk is not None and ed > kk:
            return -1, [], None
    return ed, [(0, len(y) - 1)], _cigar_of_steps(steps)


def edlib_traceback_infix(x, y, k=1):
    """(editDistance, locations, cigar) of edlib.align(x, y, mode="HW", task="path", k=k): where x sits inside y and how it aligns
    there -- what the reference's barcode-style callers of edlib_traceback(mode="HW", task="path") read.  locations holds the one
    (start, end) the other infix entry points report; the cigar is the global alignment of x against y[start:end + 1] under the tie rule
    used everywhere else (from the end: I, then D, then the diagonal).  k None or negative: unbounded.  Above k: (-1, [], None), as is
    an empty x or y.  Everything comes from the GPU (SeqStore.hw_path_pairs) and there is no host route: a machine without a GPU, or a
    pair with more than four distinct symbols, raises IsoconError, as the infix entry points do.  A name of its own, because
    edlib_traceback(mode="HW") keeps raising NotImplementedError."""
    st = SeqStore([x, y])
    try:
        rows, ops, _ = st.hw_path_pairs([0], [1], None if k is None or k < 0 else [int(k)])
    finally:
        st.close()
    TRACEBACK_INFIX_STATS["device"] += 1
    if rows[0, 0] < 0:
        return -1, [], None
    return int(rows[0, 0]), [(int(rows[0, 1]), int(rows[0, 2]))], "".join("%d%s" % (o >> 4, "=XID"[o & 15]) for o in ops.tolist())


def edlib_traceback_infix_all(x, y, k=1):
    """(editDistance, locations, cigar) of edlib.align(x, y, mode="HW", task="path", k=k) with ALL its locations: every end position of y
    at which x aligns with the best distance, in ascending order of the end, each as (start, end) with the smallest start of that
    distance (SeqStore.hw_locations) -- what primer, barcode, poly-A and repeat searches ask.  locations[0] is the one location
    edlib_traceback_infix reports, and the cigar belongs to it (edlib's convention; SeqStore.hw_path_pairs).  k None or negative:
    unbounded.  Above k, and for an empty x or y: (-1, [], None).  GPU only and at most four distinct symbols, like
    edlib_traceback_infix.  Any k is answered (SeqStore.hw_locations(wide=True)): a pair whose band max(len(y) - len(x), 0) + 2 k + 1
    fits 512 diagonals runs on the banded kernels, any other -- a 30-base primer in a 2 500-base read, any query of 256 bases or more
    with k=None -- on the un-banded ones; the limits left are those of edlib_traceback_infix."""
    kk = None if k is None or k < 0 else [int(k)]
    st = SeqStore([x, y])
    try:
        ed, loc_ptr, locs = st.hw_locations([0], [1], kk, wide=True)
        ops = st.hw_path_pairs([0], [1], kk)[1] if ed[0] >= 0 else None
    finally:
        st.close()
    TRACEBACK_INFIX_ALL_STATS["device"] += 1
    if ed[0] < 0:
        return -1, [], None
    return int(ed[0]), [(int(s), int(e)) for s, e in locs[int(loc_ptr[0]):int(loc_ptr[1])].tolist()], "".join("%d%s" % (o >> 4, "=XID"[o & 15]) for o in ops.tolist())


def edlib_traceback_prefix(x, y, k=1):
    """(editDistance, locations, cigar) of edlib.align(x, y, mode="SHW", task="path", k=k): the whole of x against a PREFIX of y -- what a
    primer or barcode search asks when the primer must sit at the read's start (on reversed strings: at its end).  editDistance is
    min over j of ed(x, y[:j]); locations holds (0, end) for every end that attains it, in ascending order (SeqStore.shw_locations);
    the cigar is the global alignment of x against y[:end + 1] for the first of them, under the tie rule used everywhere else (from the
    end: I, then D, then the diagonal; SeqStore.shw_path_pairs).  k None or negative: unbounded.  Above k, and for an empty x or y:
    (-1, [], None).  GPU only and at most four distinct symbols, like edlib_traceback_infix; a pair above distance 255 under a
    threshold beyond it raises IsoconError.  edlib_traceback(mode="SHW") keeps raising NotImplementedError."""
    kk = None if k is None or k < 0 else [int(k)]
    st = SeqStore([x, y])
    try:
        ed, end_ptr, ends = st.shw_locations([0], [1], kk)
        ops = st.shw_path_pairs([0], [1], kk)[1] if ed[0] >= 0 else None
    finally:
        st.close()
    TRACEBACK_PREFIX_STATS["device"] += 1
    if ed[0] < 0:
        return -1, [], None
    return int(ed[0]), [(0, int(e)) for e in ends[int(end_ptr[0]):int(end_ptr[1])].tolist()], "".join("%d%s" % (o >> 4, "=XID"[o & 15]) for o in ops.tolist())
