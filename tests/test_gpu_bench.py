"""GPU: a plain `python bench.py` run prints the headline line alone, and `--dump-outputs DIR` writes the graph its timed steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_the_timed_graph(tmp_path):
    import bench
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path),
           "--reads", "6000", "--length", "1200", "--isoforms", "4", "--seed", "40001"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "alignments/s" and line["dtype"] == "u64"
    assert not {"roofline", "per_rank_kernel_ms", "cpu_baseline", "other_kernels", "wrappers", "two_set_graph"} & set(line)
    best, row_ptr, cols = (np.load(tmp_path / (name + ".npy")) for name in ("best", "row_ptr", "cols"))
    assert best.dtype == row_ptr.dtype == cols.dtype == np.float64
    assert len(row_ptr) == len(best) + 1 and row_ptr[-1] == len(cols) == line["config"]["edges"]
    assert bench.graph_digest(best, row_ptr, cols) == line["config"]["graph_digest"]
