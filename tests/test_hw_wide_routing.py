"""CPU: which infix entry the pipeline asks for.  get_all_NN sets wide exactly when the widest band of its length window,
window + 2 * max_ed_allowed + 1 = 31 + 4 * ignore_ends_len, exceeds the 512 diagonals of the banded kernels (ignore_ends_len >= 121);
edlib_traceback when 2 k + 1 + max(len(y) - len(x), 0) does; dist.sharded_hw_pairs forwards the flag to every rank's store."""
import os
import random
import socket

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = []


def hw_row(O, x, y, k):
    ed, start, end = O.hw_locate(x, y, k)
    if ed < 0:
        return [-1, -1, -1, 0, 0]
    _, ops = O.nw_path(x, y[start:end + 1])
    return [ed, start, end, ops[0][0] if ops[0][1] == "I" else 0, ops[-1][0] if ops[-1][1] == "I" else 0]


class RecordingStore(object):
    """SeqStore.hw_pairs with the oracle behind it; keeps the keyword arguments of every call."""

    def __init__(self, seqs):
        self.seqs = list(seqs)
        self.lens = np.array([len(s) for s in self.seqs], dtype=np.int64)

    def hw_pairs(self, q, t, k, **kw):
        from oracle import oracle as O
        CALLS.append(dict(kw))
        kk = np.broadcast_to(np.asarray(k), (len(q),))
        return np.array([hw_row(O, self.seqs[int(a)], self.seqs[int(b)], int(c)) for a, b, c in zip(q, t, kk)], dtype=np.int32).reshape(-1, 5)


def family(seed=8):
    rng = random.Random(seed)
    full = "".join(rng.choice("ACGT") for _ in range(420))
    seqs = sorted({full[a:420 - b] for a in (0, 30, 130) for b in (0, 60, 140)}, key=len)
    return [(s, "c%d" % i) for i, s in enumerate(seqs)]


@pytest.mark.parametrize("ignore_ends_len,wide", [(0, False), (15, False), (120, False), (121, True), (150, True)])
def test_get_all_nn_sets_wide_at_the_boundary(monkeypatch, ignore_ends_len, wide):
    from isocon_amd import end_invariant_functions as END
    from oracle import oracle as O
    monkeypatch.setattr(END, "SeqStore", RecordingStore)
    del CALLS[:]
    lst = family()
    got = END.get_all_NN(lst, 0, 0, lst, 2 ** 32, ignore_ends_len)
    assert got == O.get_all_NN(lst, 0, 0, lst, 2 ** 32, ignore_ends_len)
    assert len(CALLS) == 1 and bool(CALLS[0].get("wide", False)) is wide
    assert (31 + 4 * ignore_ends_len > 512) is wide


@pytest.mark.parametrize("lx,ly,k,wide", [(100, 100, 255, False), (100, 100, 256, True), (100, 411, 100, False), (100, 412, 100, True), (300, 100, 255, False)])
def test_traceback_sets_wide_at_the_boundary(monkeypatch, lx, ly, k, wide):
    from isocon_amd import end_invariant_functions as END
    from oracle import oracle as O
    monkeypatch.setattr(END, "SeqStore", RecordingStore)
    del CALLS[:]
    rng = random.Random(lx + ly + k)
    y = "".join(rng.choice("ACGT") for _ in range(ly))
    x = (y + "".join(rng.choice("ACGT") for _ in range(lx)))[:lx]
    assert END.edlib_traceback(x, y, mode="HW", task="path", k=k, end_threshold=20) == O.edlib_traceback_hw(x, y, k=k, end_threshold=20)
    assert len(CALLS) == 1 and bool(CALLS[0].get("wide", False)) is wide


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, seqs, a, b, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from isocon_amd.dist import sharded_hw_pairs
    import test_hw_wide_routing as me
    st = me.RecordingStore(seqs)
    plain = sharded_hw_pairs(st, a, b, 12, dist=dist, device=torch.device("cpu"))
    wide = sharded_hw_pairs(st, a, b, 300, dist=dist, device=torch.device("cpu"), wide=True)
    np.savez(os.path.join(out_dir, "hw%d.npz" % rank), plain=plain, wide=wide, flags=np.array([bool(c.get("wide", False)) for c in me.CALLS]))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_hw_pairs_forwards_wide(tmp_path):
    import torch.multiprocessing as mp
    from oracle import oracle as O
    rng = random.Random(3)
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 90))) for _ in range(10)]
    seqs += [s[:10] + "A" + s[10:] for s in seqs[:5]]
    a = np.concatenate([np.array([rng.randrange(len(seqs)) for _ in range(11)], dtype=np.uint32), np.arange(5, dtype=np.uint32)])
    b = np.concatenate([np.array([rng.randrange(len(seqs)) for _ in range(11)], dtype=np.uint32), np.arange(10, 15, dtype=np.uint32)])
    mp.spawn(_worker, args=(2, _free_port(), seqs, a, b, str(tmp_path)), nprocs=2, join=True)
    plain = [hw_row(O, seqs[x], seqs[y], 12) for x, y in zip(a, b)]
    wide = [hw_row(O, seqs[x], seqs[y], 300) for x, y in zip(a, b)]
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "hw%d.npz" % r))
        assert z["plain"].tolist() == plain and z["wide"].tolist() == wide
        assert z["flags"].tolist() == [False, True]              # each rank: one call per sharded call, the flag as given
