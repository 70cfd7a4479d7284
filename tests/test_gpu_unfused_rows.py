"""The unfused scoring rows: fdx_assemble_features, and fdx_forest_prepare_features /
fdx_forest_prepare_reply (k_zfill_time, k_zfill_group, k_zfill_reply in their three row formats:
rank rows, float32 rows of 16, float32 rows of 32) followed by fdx_forest_traverse -- the entry
points of an integrator who does not use run_fused.  The reference is the feature matrix built in
numpy from the grouped columns (primitives_ref.rows_case, the input_features order of
model_training.ipynb:457-463 = pyspark/scripts/fraud_detection.py:126-132) and
oracle.forest_predict on it (scaler.transform + predict_proba, fraud_detection.py:190-193):
probabilities bit for bit, every leaf id.  W = 1, 2, 3, 4, 7 windows (7 to 31 features), with and
without a scaler, NaN amounts and averages, padding columns, NULL terminal pointers, count records
in another row order, and the documented refusals.  Workspaces and outputs start as 0x5A bytes."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
import primitives_ref as R
from fdx import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDX_E_INVALID, FDX_E_WORKSPACE = -1, -4
P = ops._ptr
# name -> (windows, set_variant or None = the library default)
FORESTS = {"w3_default": (3, None), "w3_rank_v1": (3, 1), "w3_wide16": (3, 0), "w1": (1, None), "w2": (2, None),
           "w4_wide32": (4, None), "w7_wide32": (7, None)}


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def sentinel(n, dtype, dev):
    esz = torch.empty((), dtype=dtype).element_size()
    return torch.full((n * esz,), 0x5A, dtype=torch.uint8, device=dev).view(dtype)


def untouched(buf):
    return bool((buf.contiguous().view(torch.uint8) == 0x5A).all())


@functools.lru_cache(maxsize=None)
def _case(W, scaled, nan):
    """The rows, the scaler, the forest and the oracle's answer, computed once per combination."""
    rng = np.random.default_rng(1000 * W + 10 * scaled + nan)
    d = R.rows_case(W, rng, nan_variant=nan)
    mean, scale = R.rows_scaler(d["nf"], rng) if scaled else (None, None)
    arr = R.rows_forest(d, rng, mean, scale)
    proba, leaves = oracle.forest_predict(d["X"], arr, mean, scale, want_leaves=True)
    return dict(d=d, mean=mean, scale=scale, arr=arr, proba=proba, leaves=leaves)


def _forest(c, variant):
    f = ops.Forest(c["arr"], c["d"]["nf"], c["mean"], c["scale"])
    if variant is not None:
        f.set_variant(variant)
    assert (f.variant == 0) == (c["d"]["nf"] > 15 or variant == 0)  # rank rows, or float32 rows of 16 / 32
    return f


def _inputs(d, dev):
    return dict(amount=T(d["amount"], torch.float64, dev), weekend=T(d["weekend"], torch.uint8, dev),
                night=T(d["night"], torch.uint8, dev), cust_perm=T(d["cust_perm"], torch.int32, dev),
                cust_nb=T(d["cust_nb"], torch.int32, dev), cust_avg=T(d["cust_avg"], torch.float64, dev),
                term_perm=T(d["term_perm"], torch.int32, dev), term_nb=T(d["term_nb"], torch.int32, dev),
                term_risk=T(d["term_risk"], torch.float64, dev))


def _prepare_features(f, d, t, ws, ws_bytes=None, with_terminal=True, W=None):
    tp = (P(t["term_perm"]), P(t["term_nb"]), P(t["term_risk"])) if with_terminal else (None, None, None)
    return _lib.load().fdx_forest_prepare_features(
        f._h, d["n"], d["W"] if W is None else W, P(t["amount"]), P(t["weekend"]), P(t["night"]), P(t["cust_perm"]),
        P(t["cust_nb"]), P(t["cust_avg"]), *tp, P(ws), ws.numel() if ws_bytes is None else ws_bytes, ops._s())


def _traverse(f, n, ws, dev):
    proba, leaves = sentinel(n, torch.float64, dev), sentinel(n * f.n_trees, torch.int32, dev)
    ops.check(_lib.load().fdx_forest_traverse(f._h, n, P(proba), P(leaves), P(ws), ws.numel(), ops._s()),
              "fdx_forest_traverse")
    return proba.cpu().numpy(), leaves.cpu().numpy().reshape(n, f.n_trees)


def _same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ------------------------------------------------------------------ 1. the float64 feature matrix
@pytest.mark.parametrize("nan", [False, True], ids=["base", "nan_amounts"])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 7])
def test_assemble_features(dev, W, nan):
    """X == X_ref bit for bit (NaN payloads included) with ld = width and ld = width + 5 (the
    padding keeps its bytes); with the term_* pointers NULL the terminal columns keep theirs."""
    d = _case(W, False, nan)["d"]
    t = _inputs(d, dev)
    n, nf = d["n"], d["nf"]
    L = _lib.load()
    for ld, with_terminal in ((nf, True), (nf + 5, True), (nf + 5, False), (nf, False)):
        X = sentinel(n * ld, torch.float64, dev)
        tp = (P(t["term_perm"]), P(t["term_nb"]), P(t["term_risk"])) if with_terminal else (None, None, None)
        ops.check(L.fdx_assemble_features(n, W, P(t["amount"]), P(t["weekend"]), P(t["night"]), P(t["cust_perm"]),
                                          P(t["cust_nb"]), P(t["cust_avg"]), *tp, P(X), ld, ops._s()),
                  "fdx_assemble_features")
        got = X.cpu().numpy().reshape(n, ld)
        want = np.frombuffer(b"\x5a" * 8 * n * ld, np.float64).reshape(n, ld).copy()
        keep = nf if with_terminal else 3 + 2 * W
        want[:, :keep] = d["X"][:, :keep]
        _same_bits(got, want)
    assert L.fdx_assemble_features(n, W, P(t["amount"]), P(t["weekend"]), P(t["night"]), P(t["cust_perm"]),
                                   P(t["cust_nb"]), P(t["cust_avg"]), None, None, None, P(X), nf - 1,
                                   ops._s()) == FDX_E_INVALID  # ld below the width


# ------------------------------------------------------------------ 2, 3. prepare_features + traverse
@pytest.mark.parametrize("nan", [False, True], ids=["base", "nan_amounts"])
@pytest.mark.parametrize("scaled", [False, True], ids=["raw", "scaled"])
@pytest.mark.parametrize("name", list(FORESTS))
def test_prepare_features_then_traverse(dev, name, scaled, nan):
    """Probabilities and leaf ids of the rows fdx_forest_prepare_features writes == the oracle on
    X_ref == Forest.predict(X_ref); in the NaN variant missing_go_to_left decides leaves
    (test_primitives_ref.test_rows_forest_ties_and_nan_step)."""
    W, variant = FORESTS[name]
    c = _case(W, scaled, nan)
    d = c["d"]
    f = _forest(c, variant)
    ws = sentinel(f.workspace_size(d["n"]), torch.uint8, dev)
    t = _inputs(d, dev)
    assert _prepare_features(f, d, t, ws) == 0
    proba, leaves = _traverse(f, d["n"], ws, dev)
    np.testing.assert_array_equal(leaves, c["leaves"])
    _same_bits(proba, c["proba"])
    p2, l2 = f.predict(T(d["X"], torch.float64, dev), want_leaves=True)
    _same_bits(p2.cpu().numpy(), proba)
    np.testing.assert_array_equal(l2.cpu().numpy(), leaves)


# ------------------------------------------------------------------ 4. the reply path
@pytest.mark.parametrize("scaled", [False, True], ids=["raw", "scaled"])
@pytest.mark.parametrize("name", list(FORESTS))
def test_prepare_reply_fills_the_terminal_columns(dev, name, scaled):
    """prepare_features with term_* NULL, then the terminal half from count records that arrive in
    another row order (perm), NB = 0 records among them: the same scores as the one-call form."""
    W, variant = FORESTS[name]
    c = _case(W, scaled, False)
    d = c["d"]
    n = d["n"]
    f = _forest(c, variant)
    rng = np.random.default_rng(7 + W)
    order = rng.permutation(n).astype(np.int32)  # reply record j belongs to row order[j]
    rec = R.count_records(d["tnb"][:, order], d["tfr"][:, order])
    assert ((rec & 0xFFFFFFFF) == 0).any()
    ws = sentinel(f.workspace_size(n), torch.uint8, dev)
    t = _inputs(d, dev)
    assert _prepare_features(f, d, t, ws, with_terminal=False) == 0
    recd, orderd = T(rec, torch.int64, dev), T(order, torch.int32, dev)
    ops.check(_lib.load().fdx_forest_prepare_reply(f._h, P(recd), P(orderd), n, W, 3 + 2 * W, P(ws), ws.numel(),
                                                   ops._s()), "fdx_forest_prepare_reply")
    proba, leaves = _traverse(f, n, ws, dev)
    np.testing.assert_array_equal(leaves, c["leaves"])
    _same_bits(proba, c["proba"])


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_workspace_untouched(dev):
    L = _lib.load()
    c = _case(3, True, False)
    d = c["d"]
    n, W = d["n"], 3
    t = _inputs(d, dev)
    rec = T(R.count_records(d["tnb"], d["tfr"]), torch.int64, dev)
    rows = T(np.arange(n, dtype=np.int32), torch.int32, dev)
    f = _forest(c, None)
    assert f.n_chunks == 1  # (so fdx_forest_workspace_size is exactly what the prepare calls need)
    need = f.workspace_size(n)
    ws = sentinel(need, torch.uint8, dev)

    def reply(fo, W_, col0, ws_bytes):
        return L.fdx_forest_prepare_reply(fo._h, P(rec), P(rows), n, W_, col0, P(ws), ws_bytes, ops._s())

    # a forest whose feature count is not 3 + 4W
    assert _prepare_features(f, d, t, ws, W=2) == FDX_E_INVALID
    assert _prepare_features(f, d, t, ws, W=4) == FDX_E_INVALID
    # col0 + 2W beyond the feature count
    assert reply(f, W, 3 + 2 * W + 1, need) == FDX_E_INVALID
    assert reply(f, W, -1, need) == FDX_E_INVALID
    # a workspace one byte short
    assert _prepare_features(f, d, t, ws, ws_bytes=need - 1) == FDX_E_WORKSPACE
    assert reply(f, W, 3 + 2 * W, need - 1) == FDX_E_WORKSPACE
    torch.cuda.synchronize()
    assert untouched(ws)
    # a forest in the v2 row format (the reference's deployed model: features with > 32,767 thresholds)
    z = np.load(os.path.join(ROOT, "bench_assets", "rf_deployed.npz"))
    arrays = {k: z[k].astype(np.int64) if k in ("left", "right", "feature") else z[k]
              for k in ("node_offsets", "left", "right", "feature", "threshold", "missing_left", "value1")}
    g = ops.Forest(arrays, 15, z["mean"], z["scale"])
    assert g.variant in (2, 4, 5)
    ws2 = sentinel(max(g.workspace_size(n), need), torch.uint8, dev)
    assert _prepare_features(g, d, t, ws2) == FDX_E_INVALID
    assert L.fdx_forest_prepare_reply(g._h, P(rec), P(rows), n, W, 3 + 2 * W, P(ws2), ws2.numel(),
                                      ops._s()) == FDX_E_INVALID
    torch.cuda.synchronize()
    assert untouched(ws2)
    # and the refused forest still serves the sized call
    assert _prepare_features(f, d, t, ws) == 0
    proba, leaves = _traverse(f, n, ws, dev)
    np.testing.assert_array_equal(leaves, c["leaves"])
    _same_bits(proba, c["proba"])
