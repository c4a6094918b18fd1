"""GPU: BASELINE.json configs[3]'s code path -- one process per rank, pairs sharded by ownership, min-reductions and the
all-gather of attaining edges -- driven exactly as the driver drives it: `python bench.py --gpus 2` (which starts its two
ranks itself).  No second GPU exists on the test box, so the two ranks share the one GPU and talk over gloo
(ISOCON_DIST_BACKEND=gloo); the kernels, the sharding protocol and bench.py's launcher are the real ones.  The graph must be
the one of the single-process run (digest over bounds, row pointers and neighbour order)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(n_gpus, extra_env, workload=("--reads", "6000", "--length", "1200", "--isoforms", "4", "--seed", "40001"), warmup=0):
    env = dict(os.environ)
    env.update(extra_env)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n_gpus), "--steps", "1", "--warmup", str(warmup), "--full", "--no-cpu-baseline", "--no-extras"] + list(workload)
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


@pytest.mark.timeout(900)
def test_bench_two_ranks_equal_one_rank():
    one = _bench(1, {})
    two = _bench(2, {"ISOCON_DIST_BACKEND": "gloo"})
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["rccl_ranks"] == 2 and len(two["per_rank_kernel_ms"]) == 2
    for key in ("alignments_per_step", "edges", "median_nn_distance", "graph_digest"):
        assert one["config"][key] == two["config"][key], key
    assert two["scaling"] == "strong" and two["value"] > 0


@pytest.mark.timeout(900)
def test_bench_four_real_ranks_at_configuration_size():
    """configs[3]'s launcher and collectives with REAL process groups at the size of the headline workload: `python bench.py --gpus 4` on C3
    (50 000 x 2.5 kb), four processes started by bench.py's own launcher, each with its own HIP context on the one GPU of the test box,
    torch.distributed collectives over gloo (RCCL refuses ranks that share a device) -- what the thread-baton emulation of
    tests/test_gpu_configs3.py cannot exercise.  Every rank must hold the graph of fixture g17_c3 (bench.py exits non-zero otherwise; the
    digest is asserted here too).  Four ranks, not eight: this pool allows at most six processes on a GPU box's card, and the test
    runner itself is one of them."""
    import bench
    line = _bench(4, {"ISOCON_DIST_BACKEND": "gloo"}, workload=(), warmup=1)
    assert line["n_gpus"] == 4 and line["rccl_ranks"] == 4 and line["dist_backend"] == "gloo"
    assert len(line["per_rank_kernel_ms"]) == 4 and all(ms > 0 for ms in line["per_rank_kernel_ms"])
    assert line["config"]["graph_digest"] == bench.EXPECTED_GRAPH_DIGEST_C3 and line["config"]["graph_equals_reference_loop_fixture"] is True
    assert line["config"]["edges"] == 78526 and line["scaling"] == "strong"


@pytest.mark.timeout(600)
def test_rccl_path_at_world_size_one():
    """The device-resident protocol of isocon_amd.dist with the REAL backend (nccl = RCCL): process group with device_id, the group-wide
    choice of the device path, all_reduce(MIN) on the int32 bounds in device memory, all_gather_into_tensor of the edge blocks, CSR
    from the gathered block -- with the one rank this box has (two ranks may not share a GPU under RCCL).  scripts/nccl_selfcheck.py
    compares the sharded graph, pair distances and alignments with the single calls."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "scripts", "nccl_selfcheck.py")],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
    assert out.returncode == 0 and "nccl selfcheck ok: world 1" in out.stdout, out.stdout[-3000:]
