"""The scoring step's branches that no other test runs: run_fused with two windows (the one-shot
layout without window starts, the one-pass ring kernel, the 24-byte terminal records), and
ShardedPipeline at world 1 in process (RCCL) in both avg modes, against FraudPipeline on the same
rows -- the probabilities, the featurized table, featurize, and the id-range check."""
import os
import socket

import numpy as np
import pytest
import torch

from fdx import _lib, ops, synth
from fdx.pipeline import FraudPipeline
from forest_gen import random_forest
from table_check import table_as_X

pytestmark = pytest.mark.gpu
N_CUST, N_TERM, DAYS = 800, 1600, 20
COLS = ("ts", "customer", "terminal", "amount", "fraud")


@pytest.fixture(scope="module")
def table(dev):
    g = synth.generate_device(N_CUST, N_TERM, DAYS, seed=41, device=dev)
    assert 2000 < g["ts"].numel() < 100_000
    return tuple(g[k] for k in COLS)


@pytest.fixture(scope="module")
def world1(dev):
    """The NCCL world-1 group of test_gpu_edge.py::test_sharded_rank_without_rows."""
    import torch.distributed as dist

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]))
    s.close()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _forest15(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def test_run_fused_two_windows(dev, table):
    """W = 2: proba of the fused step == score(featurize(...).X) bit for bit; the second step on the
    same pipeline takes the layout's slot hint."""
    rng = np.random.default_rng(11)
    arrays = random_forest(rng, 5, 6, n_feat=11)
    # (amount, weekend, night, customer nb / avg x 2, terminal nb / risk x 2: scales near the data's)
    mean = np.array([50, .5, .5, 2, 50, 10, 50, 1, .1, 5, .1]) * rng.uniform(0.8, 1.2, 11)
    scale = np.array([30, .5, .5, 2, 30, 10, 30, 1, .1, 5, .1]) * rng.uniform(0.8, 1.2, 11)
    pipe = FraudPipeline(windows_days=(1, 7), forest=ops.Forest(arrays, 11, mean, scale))
    X = pipe.featurize(*table, N_CUST, N_TERM).X
    assert X.shape == (table[0].numel(), 11)
    want = pipe.score(X).cpu().numpy()
    assert len(np.unique(want)) > 1
    for step in range(2):
        p = torch.full((table[0].numel(),), -1.0, dtype=torch.float64, device=dev)
        pipe.run_fused(*table, N_CUST, N_TERM, p)
        np.testing.assert_array_equal(p.cpu().numpy(), want, err_msg=f"step {step}")


@pytest.mark.parametrize("avg_mode", ("exact", "scan"))
def test_sharded_world1_equals_single_gpu(dev, golden, table, world1, avg_mode):
    from fdx.distributed import ShardedPipeline

    forest = _forest15(golden)
    n = table[0].numel()
    amount = table[3].cpu().numpy()
    cap = n * 11 // 10 + 4096
    ref = FraudPipeline(forest=forest, avg_mode=avg_mode)
    p_ref = torch.empty(n, dtype=torch.float64, device=dev)
    r_ref = ops.FeatureTable(cap, dev)
    ref.run_fused(*table, N_CUST, N_TERM, p_ref, rows_out=r_ref)
    torch.cuda.synchronize()
    X_ref = table_as_X(r_ref, ref.last_slots, amount)
    sp = ShardedPipeline(FraudPipeline(forest=forest, avg_mode=avg_mode), 1, 0, N_TERM, customer_base=0,
                         n_customers_local=N_CUST)
    for step in range(2):  # (the second step reuses the side stream, the arena and the slot hint)
        p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        rows = ops.FeatureTable(cap, dev)
        sp.run(*table, p, ops.workspace(forest.workspace_size(cap), dev), rows_out=rows)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(p.cpu().numpy(), p_ref.cpu().numpy(), err_msg=f"step {step} proba")
        np.testing.assert_array_equal(table_as_X(rows, sp.pipe.last_slots, amount).view(np.int64),
                                      X_ref.view(np.int64), err_msg=f"step {step} featurized table")
    X = sp.featurize(*table)
    X_one = FraudPipeline(forest=forest, avg_mode=avg_mode).featurize(*table, N_CUST, N_TERM).X
    np.testing.assert_array_equal(X.cpu().numpy().view(np.int64), X_one.cpu().numpy().view(np.int64))
    # one id past this rank's range: refused, by name
    cust = table[1].clone()
    cust[5] = N_CUST
    p = torch.empty(n, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.FdxError, match="customer ids"):
        sp.run(table[0], cust, *table[2:], p, ops.workspace(forest.workspace_size(cap), dev))
    torch.cuda.synchronize()
