"""bench.py on the MI355X: a plain run (no --full) prints the timed line only, and --dump-outputs writes what its last
timed step computed -- checked here against SciPy on the same seeded inputs."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    import bench
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "reddit-small", "--dump-outputs", str(tmp_path)]
    line = bench.main(argv)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["metric"] == "training edges/s (SpMM)" and line["unit"] == "edges/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True
    # the legs of --full did not run
    assert not {"setup", "cpu_baseline", "train_epoch", "strong"} & set(line) and "traffic_live" not in line["roofline"]
    assert sorted(os.listdir(str(tmp_path))) == ["C.npy", "dX.npy"]
    C, dX = np.load(str(tmp_path / "C.npy")), np.load(str(tmp_path / "dX.npy"))
    assert C.dtype == np.float32 and dX.dtype == np.float32 and C.nbytes + dX.nbytes <= bench.DUMP_BUDGET
    # the same inputs bench.main builds: rank 0's graph, then X and dC from one device generator seeded 1234
    n, full_adj, _, _ = bench.make_graph(bench.parse(argv), 0)
    d = line["config"]["d"]
    assert C.shape[1] == d and dX.shape == C.shape and 0 < C.shape[0] <= n
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234)
    X = torch.randn((n, d), device="cuda:0", generator=gen).cpu().numpy()
    dC = torch.randn((n, d), device="cuda:0", generator=gen).cpu().numpy()
    rows = np.arange(n) if C.shape[0] == n else \
        np.sort(np.random.RandomState(bench.DUMP_SEED).choice(n, C.shape[0], replace=False))
    assert onp.rel_err(C, full_adj[rows].dot(X)) <= 1e-4
    assert onp.rel_err(dX, full_adj.T.tocsr()[rows].dot(dC)) <= 1e-4
