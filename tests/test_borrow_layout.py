"""Rank layout v3, "borrow" nodes (host only, no GPU): fdx_forest_pack_rank2(version=3) walked by a
numpy model of the kernel's step in exactly its 32-bit arithmetic,

    x  = slot << 28 | rank                   (the row's plane word; NaN: low half 0xFFFF)
    d  = node - x                            (uint32; the slot bits cancel, borrow iff rank > k)
    p += d >> 16                             (= O - (rank > k); the kernel's v_mad_u32_u16)
    next slot = node >> 28, a leaf iff node & 0x0FFF0000 == 0,

must give sklearn's leaves and probabilities bit for bit, and the layout must have the structure
include/fdx.h documents (sibling pairs, O >= 2, fixed-point leaves, O <= 4095 or refusal)."""
import ctypes
import os

import numpy as np
import pytest

import oracle
from forest_gen import random_forest
from test_rank_layout import _desc, _z32, pack_rank, pack_rank2

LEAF = np.uint32(0x00007FFF)
O_MASK = np.uint32(0x0FFF0000)
FDX_E_UNSUPPORTED = -3


def planes(R, z32):
    """[n, 15] uint32 plane words of the rows."""
    n = z32.shape[0]
    x = np.zeros((n, 15), np.uint32)
    for f in range(15):
        col = z32[:, f] if f < z32.shape[1] else np.zeros(n, np.float32)
        u = R["thr"][R["thr_off"][f]:R["thr_off"][f + 1]]
        r = np.searchsorted(u, col, side="left").astype(np.uint32)
        r[np.isnan(col)] = 0xFFFF
        x[:, f] = (np.uint32(f) << np.uint32(28)) | r
    return x


def walk_borrow(R, z32, trees=None):
    x = planes(R, z32)
    n = len(x)
    rows = np.arange(n)
    nodes = R["nodes"].astype(np.uint32)
    trees = range(len(R["root"])) if trees is None else trees
    acc = np.zeros(n)
    leaves = np.zeros((n, len(trees)), np.int32)
    for j, t in enumerate(trees):
        p = np.full(n, R["root"][t], np.int64)
        for _ in range(int(R["depth"][t])):
            nd = nodes[p]
            xv = x[rows, nd >> np.uint32(28)]
            st = (nd - xv) >> np.uint32(16)  # uint32 wrap-around subtraction
            o = (nd >> np.uint32(16)) & np.uint32(0xFFF)
            st_nan = np.where(o == 0, 0, o - (R["ml"][p] == 0))  # missing_go_to_left; a leaf stays
            p = p + np.where((xv & np.uint32(0xFFFF)) == 0xFFFF, st_nan, st)
        assert ((nodes[p] & O_MASK) == 0).all(), "walk did not end on leaves within depth"
        acc = acc + R["lval"][p]
        leaves[:, j] = R["orig"][p]
    return acc / len(trees), leaves


def check_structure(a, R):
    """Sibling pairs (right = left - 1 at p + O - 1, p + O), O in [2, 4095], leaves 0x7FFF, the word
    count = the node count, k / k + 1 straddle every branch, orig / missing_left / values by word."""
    nodes = R["nodes"].astype(np.uint32)
    off = a["node_offsets"]
    assert len(nodes) == off[-1]
    ends = np.append(R["root"][1:], len(nodes))
    for t, (b, e) in enumerate(zip(R["root"], ends)):
        assert e - b == off[t + 1] - off[t]
        nd, orig = nodes[b:e], R["orig"][b:e].astype(np.int64)
        assert sorted(orig) == list(range(e - b)) and orig[0] == 0
        left, right = a["left"][off[t]:off[t + 1]], a["right"][off[t]:off[t + 1]]
        internal = left[orig] >= 0
        np.testing.assert_array_equal((nd & O_MASK) != 0, internal)
        assert (nd[~internal] == LEAF).all()
        np.testing.assert_array_equal(R["lval"][b:e][~internal], a["value1"][off[t]:off[t + 1]][orig[~internal]])
        p = np.nonzero(internal)[0]
        w = nd[p]
        o = ((w >> np.uint32(16)) & np.uint32(0xFFF)).astype(np.int64)
        s, k = w >> np.uint32(28), w & np.uint32(0xFFFF)
        assert (o >= 2).all() and (o <= 4095).all() and (k <= 0x7FFE).all() and (s <= 14).all()
        assert (o <= (e - b) // 2 + 2).all()
        np.testing.assert_array_equal(orig[p + o], left[orig[p]])
        np.testing.assert_array_equal(orig[p + o - 1], right[orig[p]])
        np.testing.assert_array_equal(s, a["feature"][off[t]:off[t + 1]][orig[p]])
        np.testing.assert_array_equal(R["ml"][b:e][p], a["missing_left"][off[t]:off[t + 1]][orig[p]])
        sw = s << np.uint32(28)
        np.testing.assert_array_equal((w - (sw | k)) >> np.uint32(16), o)  # rank k: left
        np.testing.assert_array_equal((w - (sw | (k + np.uint32(1)))) >> np.uint32(16), o - 1)  # k + 1: right
        np.testing.assert_array_equal((w - sw) >> np.uint32(16), o)  # rank 0
        np.testing.assert_array_equal((w - (sw | np.uint32(0x7FFF))) >> np.uint32(16), o - 1)  # rank 0x7FFF


def test_leaf_is_a_fixed_point_under_every_rank():
    r = np.arange(0x8000, dtype=np.uint32)
    assert ((LEAF - r) >> np.uint32(16) == 0).all()  # slot 0's plane word is the rank itself
    assert LEAF & O_MASK == 0 and LEAF >> np.uint32(28) == 0


@pytest.mark.parametrize("name", ["forest_dt2.npz", "forest_rf5d8.npz", "forest_rf3.npz"])
def test_borrow_layout_reproduces_sklearn(golden, name):
    z = golden(name)
    R = pack_rank2(z, version=3)
    assert R is not None
    check_structure(z, R)
    proba, leaves = walk_borrow(R, _z32(z["X"], z["mean"], z["scale"]))
    np.testing.assert_array_equal(leaves, z["leaves"])
    np.testing.assert_array_equal(proba, z["proba"])
    # the same rows with NaNs: missing_go_to_left against the C oracle
    rng = np.random.default_rng(4)
    X = np.array(z["X"], np.float64)
    X[rng.random(X.shape) < 0.1] = np.nan
    arr = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    op, ol = oracle.forest_predict(X, arr, z["mean"], z["scale"], want_leaves=True)
    proba, leaves = walk_borrow(R, _z32(X, z["mean"], z["scale"]))
    np.testing.assert_array_equal(leaves, ol)
    np.testing.assert_array_equal(proba, op)


@pytest.mark.parametrize("depth", list(range(0, 11)))
def test_borrow_layout_random_forests(depth):
    """Depth 0 = single-leaf trees, 1 = stumps, up to 10; NaN rows included."""
    rng = np.random.default_rng(100 + depth)
    a = random_forest(rng, 7, depth, p_leaf=0.2)
    R = pack_rank2(a, version=3)
    assert R is not None
    check_structure(a, R)
    assert max(R["depth"]) == depth
    X = rng.normal(size=(1500, 15))
    X[rng.random(X.shape) < 0.05] = np.nan
    op, ol = oracle.forest_predict(X, a, want_leaves=True)
    proba, leaves = walk_borrow(R, X.astype(np.float32))
    np.testing.assert_array_equal(leaves, ol)
    np.testing.assert_array_equal(proba, op)


def test_borrow_layout_bench_model():
    from conftest import ROOT

    z = np.load(os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    R = pack_rank2(z, version=3)
    assert R is not None and len(R["nodes"]) == z["node_offsets"][-1]
    check_structure(z, R)
    proba, _ = walk_borrow(R, _z32(z["check_X"], z["mean"], z["scale"]))
    np.testing.assert_array_equal(proba, z["check_proba"])


def test_borrow_extreme_ranks():
    """32,767 stumps on feature 0 with distinct thresholds: tree j tests k = j, so k = 0 and k =
    0x7FFE both occur; rows at the threshold (rank k, left) and one float above (rank k + 1, right;
    0x7FFF for the last tree) take the oracle's side."""
    n = 32767
    thr = np.arange(n, dtype=np.float64) / 64.0
    a = dict(node_offsets=np.arange(0, 3 * n + 1, 3, dtype=np.int64),
             left=np.tile(np.array([1, -1, -1], np.int64), n), right=np.tile(np.array([2, -1, -1], np.int64), n),
             feature=np.tile(np.array([0, -2, -2], np.int64), n), threshold=np.repeat(thr, 3),
             missing_left=np.zeros(3 * n, np.uint8), value1=np.tile(np.array([0.0, 0.25, 0.75]), n))
    R = pack_rank2(a, version=3)
    assert R is not None
    k = R["nodes"][R["root"]] & 0xFFFF
    np.testing.assert_array_equal(k, np.arange(n))
    trees = [0, 1, n - 2, n - 1]
    cand = np.concatenate([[-1.0], thr[trees], np.nextafter(thr[trees].astype(np.float32), np.float32(np.inf)), [1e9]])
    z32 = np.zeros((len(cand), 15), np.float32)
    z32[:, 0] = cand
    x0 = planes(R, z32)[:, 0]
    assert x0.min() == 0 and x0.max() == 0x7FFF
    _, leaves = walk_borrow(R, z32, trees)
    expect = np.where(z32[:, :1].astype(np.float64) <= thr[trees][None, :], 1, 2)
    np.testing.assert_array_equal(leaves, expect)


def test_borrow_layout_refuses_far_children():
    """A complete depth-12 tree (8,191 nodes): the root's second child's pair lies past 4,095 words,
    so v3 refuses the forest with FDX_E_UNSUPPORTED; v1 (jump nodes) holds it."""
    from fdx import _lib

    rng = np.random.default_rng(12)
    a = random_forest(rng, 1, 12, p_leaf=0.0)
    assert a["node_offsets"][-1] == 8191
    L = _lib.load()
    d, keep = _desc(a, 15)
    nn, nthr, ns = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    rc = L.fdx_forest_rank_layout_size2(ctypes.byref(d), 3, ctypes.byref(nn), ctypes.byref(nthr), ctypes.byref(ns))
    assert rc == FDX_E_UNSUPPORTED
    assert pack_rank(a) is not None
    b = random_forest(rng, 1, 11, p_leaf=0.0)  # 4,095 nodes: O <= 2,049
    R = pack_rank2(b, version=3)
    assert R is not None
    check_structure(b, R)
