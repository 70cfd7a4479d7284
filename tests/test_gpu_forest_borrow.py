"""Variant 6 of the forest walk: rank layout v3 ("borrow" sibling-pair nodes, include/fdx.h) through
k_forest_rank's tile loops.  Probabilities bit-equal and leaf ids equal to the wide-layout kernel
(variant 0) and the C oracle of sklearn's Tree._apply_dense: the golden forests with and without NaN
rows, random forests of 1-8 and 13 trees at depths 0, 1, 4 and 9, row counts around the wave and
tile sizes; the bench model on its check rows; run_fused against variant 1; set_variant to and from
the format, and a refused switch.
Reference call: pyspark/scripts/fraud_detection.py:190-193 (predict_proba of the loaded model)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from fdx import _lib, ops, synth
from fdx._lib import FdxError
from fdx.pipeline import FraudPipeline
from forest_gen import random_forest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORROW = 6
COUNTS = [1, 63, 64, 65, 1024, 1025, 3 * 1024 + 7]
KEYS = ("node_offsets", "left", "right", "feature", "threshold", "missing_left", "value1")


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def _arrays(z):
    return {k: z[k].astype(np.int64) if k in ("left", "right", "feature") else z[k] for k in KEYS}


V3, V1 = (1, 15), (1, 16)  # fdx_forest_layout: v1 rows and u32 planes; v3 has no sentinel slot


def _layout(f):
    lay, ns = ctypes.c_int32(), ctypes.c_int32()
    assert _lib.load().fdx_forest_layout(f._h, ctypes.byref(lay), ctypes.byref(ns)) == 0
    return lay.value, ns.value


def _check_counts(f, g, X, arr, mean, scale, dev):
    """f (variant 6) on every prefix of X in COUNTS == g (variant 0) and the oracle, leaf ids too."""
    want_p, want_l = oracle.forest_predict(X, arr, mean, scale, want_leaves=True)
    Xd = T(X, torch.float64, dev)
    gp, gl = g.predict(Xd, want_leaves=True)
    np.testing.assert_array_equal(gp.cpu().numpy(), want_p)
    for n in COUNTS:
        p, leaves = f.predict(Xd[:n], want_leaves=True)
        assert torch.equal(p, gp[:n]) and torch.equal(leaves, gl[:n]), n
        assert torch.equal(f.predict(Xd[:n]), gp[:n]), n  # without leaf ids: the one-group loops
        np.testing.assert_array_equal(leaves.cpu().numpy(), want_l[:n])


@pytest.mark.parametrize("name", ["forest_dt2.npz", "forest_rf3.npz", "forest_rf5d8.npz"])
def test_borrow_golden_forests(dev, golden, name):
    z = golden(name)
    arr = _arrays(z)
    f = ops.Forest(arr, 15, z["mean"], z["scale"])
    assert f.variant == BORROW and _layout(f) == V3
    g = ops.Forest(arr, 15, z["mean"], z["scale"])
    g.set_variant(0)
    reps = -(-COUNTS[-1] // len(z["X"]))
    X = np.vstack([z["X"]] * reps)[:COUNTS[-1]]
    p = f.predict(T(X, torch.float64, dev)).cpu().numpy()
    np.testing.assert_array_equal(p, np.concatenate([z["proba"]] * reps)[:COUNTS[-1]])  # sklearn's own
    _check_counts(f, g, X, arr, z["mean"], z["scale"], dev)
    Xn = X.copy()
    Xn[np.random.default_rng(6).random(Xn.shape) < 0.05] = np.nan
    _check_counts(f, g, Xn, arr, z["mean"], z["scale"], dev)


@pytest.mark.parametrize("n_trees", [1, 2, 3, 4, 5, 6, 7, 8, 13])
def test_borrow_random_forests(dev, n_trees):
    """Depth 0 (single leaves) and 1 (stumps: the first step is the read-free last one) included;
    13 trees: more than one walk group."""
    for depth in (0, 1, 4, 9):
        rng = np.random.default_rng(100 * n_trees + depth)
        arr = random_forest(rng, n_trees, depth, p_leaf=0.1)
        f = ops.Forest(arr, 15)
        f.set_variant(BORROW)
        assert _layout(f) == V3
        g = ops.Forest(arr, 15)
        g.set_variant(0)
        X = rng.normal(size=(COUNTS[-1], 15))
        _check_counts(f, g, X, arr, None, None, dev)
        X[rng.random(X.shape) < 0.05] = np.nan
        _check_counts(f, g, X, arr, None, None, dev)


def test_borrow_several_chunks(dev):
    """20 trees of depth 12 (several LDS chunks: the chunk loop, and one launch per chunk with leaf
    ids) on 300k rows, NaN rows too."""
    rng = np.random.default_rng(77)
    arr = random_forest(rng, 20, 12, p_leaf=0.05)
    f = ops.Forest(arr, 15)
    assert f.variant == BORROW and f.n_chunks > 1
    g = ops.Forest(arr, 15)
    g.set_variant(0)
    n = 300_017
    X = rng.normal(size=(n, 15))
    for Xi in (X, np.where(rng.random(X.shape) < 0.03, np.nan, X)):
        Xd = T(Xi, torch.float64, dev)
        p = f.predict(Xd)
        gp, gl = g.predict(Xd, want_leaves=True)
        assert torch.equal(p, gp)
        pl, leaves = f.predict(Xd, want_leaves=True)
        assert torch.equal(pl, gp) and torch.equal(leaves, gl)
        sel = rng.choice(n, 5000, replace=False)
        np.testing.assert_array_equal(p.cpu().numpy()[sel], oracle.forest_predict(Xi[sel], arr))


def test_borrow_bench_model_check_rows(dev):
    z = np.load(os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    f = ops.Forest(_arrays(z), 15, z["mean"], z["scale"])
    assert f.variant == BORROW and _layout(f) == V3 and f.n_chunks == 18
    assert len(z["check_X"]) == 4096
    p = f.predict(T(z["check_X"], torch.float64, dev)).cpu().numpy()
    np.testing.assert_array_equal(p, z["check_proba"])
    # past the all-chunks-at-once size: the one-launch chunk loop
    reps = 80
    assert f.traverse_launches(reps * 4096) == 1
    pc = f.predict(T(np.vstack([z["check_X"]] * reps), torch.float64, dev)).cpu().numpy()
    np.testing.assert_array_equal(pc, np.concatenate([z["check_proba"]] * reps))


def test_borrow_run_fused_equals_variant_1(dev, golden):
    """A 2,000-customer, 30-day table through run_fused with the new default and with variant 1:
    the same probabilities and the same feature table, byte for byte."""
    z = golden("forest_rf5d8.npz")
    d = synth.generate(2000, 1000, 30, seed=9)
    args = (T(d["ts"], torch.int64, dev), T(d["customer"], torch.int32, dev), T(d["terminal"], torch.int32, dev),
            T(d["amount"], torch.float64, dev), T(d["fraud"], torch.uint8, dev), 2000, 1000)
    n = len(d["ts"])
    out = {}
    for v in (BORROW, 1):
        f = ops.Forest(_arrays(z), 15, z["mean"], z["scale"])
        assert f.variant == BORROW
        f.set_variant(v)
        pipe = FraudPipeline(forest=f)
        rows = ops.FeatureTable((2 * n + 4096 + 63) // 64 * 64, dev)
        rows.buf.fill_(0x5A)
        assert f.in_table_ok(3, rows)
        proba = torch.empty(n, dtype=torch.float64, device=dev)
        pipe.run_fused(*args, proba, rows_out=rows)
        torch.cuda.synchronize()
        out[v] = (proba, rows.buf, pipe.last_slots)
    assert out[BORROW][2] == out[1][2]
    assert torch.equal(out[BORROW][0], out[1][0])
    assert torch.equal(out[BORROW][1], out[1][1])
    assert bool((out[1][0] >= 0).all()) and bool((out[1][0] > 0).any())


def test_borrow_set_variant_round_trips(dev, golden):
    """(every feature of this forest fits one v2 slot, so its v2 form reports layout 3)"""
    z = golden("forest_rf5d8.npz")
    f = ops.Forest(_arrays(z), 15, z["mean"], z["scale"])
    X = T(z["X"], torch.float64, dev)
    for v, lay in ((BORROW, V3), (1, V1), (BORROW, V3), (2, (3, 15)), (BORROW, V3), (3, (3, 15)), (0, (3, 15)),
                   (BORROW, V3)):
        f.set_variant(v)
        assert f.variant == v and _layout(f) == lay
        p, leaves = f.predict(X, want_leaves=True)
        np.testing.assert_array_equal(p.cpu().numpy(), z["proba"])
        np.testing.assert_array_equal(leaves.cpu().numpy(), z["leaves"])


def test_borrow_refused_leaves_the_forest_intact(dev):
    """A complete depth-12 tree (8,191 nodes) has a child pair more than 4,095 words from its parent:
    the forest builds as v1, set_variant(6) is refused and leaves it as it was."""
    rng = np.random.default_rng(12)
    arr = random_forest(rng, 1, 12, p_leaf=0.0)
    f = ops.Forest(arr, 15)
    assert f.variant == 1 and _layout(f) == V1
    nc = f.n_chunks
    X = rng.normal(size=(5000, 15))
    X[rng.random(X.shape) < 0.02] = np.nan
    want = oracle.forest_predict(X, arr)
    for _ in range(2):
        with pytest.raises(FdxError):
            f.set_variant(BORROW)
        assert f.variant == 1 and _layout(f) == V1 and f.n_chunks == nc
        np.testing.assert_array_equal(f.predict(T(X, torch.float64, dev)).cpu().numpy(), want)
