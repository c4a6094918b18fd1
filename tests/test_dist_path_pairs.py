"""CPU, world_size 2, gloo: alignment paths of a pair list over several ranks (isocon_amd.dist.sharded_path_pairs) -- the round-robin
shards, the agreement check and the ragged gathers -- with the device work replaced by an oracle-backed stand-in that keeps the
contracts of SeqStore.ed_path_pairs (global paths) and SeqStore.hw_path_pairs (infix paths)."""
import os
import random
import re
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

CODE = {"=": 0, "X": 1, "I": 2, "D": 3}


class FakePathStore(object):
    """SeqStore.ed_path_pairs / hw_path_pairs with the CPU oracle behind them."""

    def __init__(self, seqs):
        self.seqs = seqs
        self.lens = np.array([len(s) for s in seqs], dtype=np.int64)

    def ed_path_pairs(self, q, t, k=None):
        from oracle import oracle as O
        kk = np.broadcast_to(np.asarray(-1 if k is None else k), (len(q),))
        ed, ops, ptr = [], [], [0]
        for x, y, kp in zip(q, t, kk):
            d, path = O.nw_path(self.seqs[int(x)], self.seqs[int(y)])
            if 0 <= int(kp) < d:
                d, path = -1, []
            ed.append(d)
            ops += [(ln << 4) | CODE[c] for ln, c in path]
            ptr.append(len(ops))
        return np.array(ed, dtype=np.int32), np.array(ops, dtype=np.uint32), np.array(ptr, dtype=np.uint64)

    def hw_path_pairs(self, q, t, k=None):
        from oracle import oracle as O
        kk = np.broadcast_to(np.asarray(-1 if k is None else k), (len(q),))
        rows, ops, ptr = [], [], [0]
        for x, y, kp in zip(q, t, kk):
            a, b = self.seqs[int(x)], self.seqs[int(y)]
            r = O.hw_path(a, b, int(kp) if int(kp) >= 0 else len(a)) if a and b else {"cigar": None}
            if r["cigar"] is None:
                rows.append([-1, -1, -1, 0, 0])
            else:
                path = [(int(ln), c) for ln, c in re.findall(r"(\d+)([=XID])", r["cigar"])]
                start, end = r["locations"][0]
                rows.append([r["editDistance"], start, end, path[0][0] if path[0][1] == "I" else 0, path[-1][0] if path[-1][1] == "I" else 0])
                ops += [(ln << 4) | CODE[c] for ln, c in path]
            ptr.append(len(ops))
        return np.array(rows, dtype=np.int32).reshape(-1, 5), np.array(ops, dtype=np.uint32), np.array(ptr, dtype=np.uint64)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import sys
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _worker(rank, world, port, seqs, a, b, k, out_dir):
    _init(rank, world, port)
    from isocon_amd.dist import sharded_path_pairs
    st = FakePathStore(seqs)
    cpu = torch.device("cpu")
    ed, ops, ptr = sharded_path_pairs(st, a, b, k, dist=dist, device=cpu)
    ed_u, ops_u, ptr_u = sharded_path_pairs(st, a, b, dist=dist, device=cpu)
    rows, hops, hptr = sharded_path_pairs(st, a, b, k, infix=True, dist=dist, device=cpu)
    np.savez(os.path.join(out_dir, "paths%d.npz" % rank), ed=ed, ops=ops, ptr=ptr, ed_u=ed_u, ops_u=ops_u, ptr_u=ptr_u, rows=rows, hops=hops, hptr=hptr)
    dist.barrier()
    dist.destroy_process_group()


def pair_list():
    """29 pairs of mixed sizes: random ones (misses under k = 12), sequences with a variant of theirs, slices inside their sequence"""
    rng = random.Random(5)
    seqs = ["".join(rng.choice("ACGT") for _ in range(rng.randint(20, 150))) for _ in range(12)]
    seqs += [s[:10] + "A" + s[10:] for s in seqs[:5]]                      # 12 .. 16: one insertion
    seqs += [s[7:len(s) - 9] for s in seqs[5:10]]                          # 17 .. 21: a slice
    seqs += [seqs[10][3:15] + "T" + seqs[10][15:len(seqs[10]) - 2]]        # 22: a slice with an edit
    a = [rng.randrange(len(seqs)) for _ in range(13)] + list(range(5)) + list(range(17, 22)) + [22] + list(range(12, 17))
    b = [rng.randrange(len(seqs)) for _ in range(13)] + list(range(12, 17)) + list(range(5, 10)) + [10] + list(range(5))
    return seqs, np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)


def test_sharded_path_pairs_two_ranks(tmp_path):
    seqs, a, b = pair_list()
    assert len(a) == 29
    k = np.full(29, 12, dtype=np.int32)
    mp.spawn(_worker, args=(2, _free_port(), seqs, a, b, k, str(tmp_path)), nprocs=2, join=True)
    st = FakePathStore(seqs)
    ed, ops, ptr = st.ed_path_pairs(a, b, k)
    ed_u, ops_u, ptr_u = st.ed_path_pairs(a, b)
    rows, hops, hptr = st.hw_path_pairs(a, b, k)
    assert (rows[:, 0] >= 0).sum() >= 3 and (rows[:, 0] < 0).sum() >= 3 and (ed >= 0).sum() >= 3 and (ed < 0).sum() >= 3
    assert (rows[:, 1] > 0).sum() >= 3                                   # infix hits that do not begin at the target's first base
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "paths%d.npz" % r))
        for name, want in (("ed", ed), ("ops", ops), ("ptr", ptr), ("ed_u", ed_u), ("ops_u", ops_u), ("ptr_u", ptr_u), ("rows", rows), ("hops", hops),
                           ("hptr", hptr)):
            assert z[name].dtype == want.dtype and z[name].shape == want.shape and (z[name] == want).all(), (r, name)


def _worker_differ(rank, world, port, seqs, a, b, out_dir):
    _init(rank, world, port)
    from isocon_amd.dist import sharded_path_pairs
    st = FakePathStore(seqs)
    if rank == 1:
        a = a.copy()
        a[4], a[5] = a[5], a[4]
    said = []
    for infix in (False, True):
        try:
            sharded_path_pairs(st, a, b, 12, infix=infix, dist=dist, device=torch.device("cpu"))
            said.append("no error")
        except RuntimeError as e:
            said.append(str(e))
    open(os.path.join(out_dir, "differ%d.txt" % rank), "w").write("\n".join(said))
    dist.barrier()
    dist.destroy_process_group()


def test_ranks_with_different_lists_raise(tmp_path):
    seqs, a, b = pair_list()
    assert a[4] != a[5]
    mp.spawn(_worker_differ, args=(2, _free_port(), seqs, a, b, str(tmp_path)), nprocs=2, join=True)
    for r in (0, 1):
        said = open(tmp_path / ("differ%d.txt" % r)).read().splitlines()
        assert len(said) == 2 and all("the ranks hold different pair lists" in s for s in said)
