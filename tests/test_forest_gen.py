"""forest_gen's exact-count forests and edge rows (host only, no GPU): what the GPU tests of the
rank search tables (test_gpu_rank_tables.py) rely on -- the library sees exactly the threshold
counts a case names, the shapes written in RANK_CASES follow from the formats' rules, every
(at a threshold, just above it) pair of edge rows scores differently in the oracle, so that a rank
that is off by one there cannot hide, and the fused step's table reaches the table edges."""
import ctypes

import numpy as np
import pytest

import oracle
from forest_gen import (RANK_CASES, SEARCHED, SLOT_SPAN, edge_ranks, expected_tables, rank_case, table_edge_report,
                        threshold_forest)
from test_rank_layout import _desc


@pytest.fixture(scope="module", params=list(RANK_CASES))
def case(request):
    return rank_case(request.param)


def test_written_shapes_follow_from_the_rules():
    for name, (counts, (seg, n_samples, n_tree_floats, levels)) in RANK_CASES.items():
        assert len(counts) == 15
        assert expected_tables(counts, max(counts) > SLOT_SPAN) == dict(seg=seg, n_samples=n_samples,
                                                                       n_tree_floats=n_tree_floats,
                                                                       tree_levels=levels), name
    # the steps the cases are about: one threshold more than a full table doubles the segment
    assert expected_tables(RANK_CASES["v1_full"][0])["n_samples"] == 8192
    assert expected_tables(RANK_CASES["v2_full"][0], True)["n_samples"] == 20480
    # an identity v2 forest has v1 rows: the v1 budget, not v2's (the same forest under both)
    one_more = RANK_CASES["v1_one_more"][0]
    assert expected_tables(one_more, False)["seg"] == 32 and expected_tables(one_more, True)["seg"] == 16


def test_threshold_counts_are_exact(case):
    """Through fdx_forest_rank_layout_size2 (the totals, v2's slots; v1 / v3 refuse a feature with
    more than 32,767 thresholds) and fdx_forest_pack_rank2 (per feature, and the values)."""
    from fdx import _lib

    L = _lib.load()
    counts, U = case["counts"], case["thresholds"]
    d, keep = _desc(case["arrays"], 15)
    nn, nthr, ns = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    for version in (1, 2, 3):
        rc = L.fdx_forest_rank_layout_size2(ctypes.byref(d), version, ctypes.byref(nn), ctypes.byref(nthr),
                                            ctypes.byref(ns))
        if version != 2 and case["v2"]:
            assert rc == _lib.FDX_E_UNSUPPORTED and b"distinct thresholds" in L.fdx_last_error()
            continue
        assert rc == 0, L.fdx_last_error()
        assert nthr.value == sum(counts)
        assert ns.value == (sum(max(1, -(-c // SLOT_SPAN)) for c in counts) if version == 2 else 16)
    n, nt = nn.value, d.n_trees  # (version 3 or 2: the last one sized)
    out = dict(nodes=np.zeros(n, np.uint32), orig=np.zeros(n, np.int32), lval=np.zeros(n), ml=np.zeros(n, np.uint8),
               root=np.zeros(nt, np.int32), depth=np.zeros(nt, np.int32), thr=np.zeros(max(nthr.value, 1), np.float32),
               thr_off=np.zeros(33, np.int32), slot_feat=np.zeros(32, np.int32), slot_base=np.zeros(32, np.int32))
    assert L.fdx_forest_pack_rank2(ctypes.byref(d), 2 if case["v2"] else 3, *[out[k].ctypes.data for k in
                                   ("nodes", "orig", "lval", "ml", "root", "depth", "thr", "thr_off", "slot_feat",
                                    "slot_base")]) == 0, L.fdx_last_error()
    for f in range(15):
        got = out["thr"][out["thr_off"][f]:out["thr_off"][f + 1]]
        assert len(got) == counts[f] == len(U[f])
        np.testing.assert_array_equal(got, U[f])
    # a tenth of the thresholds lie between two float32 values; leaf values are distinct within a tree
    a = case["arrays"]
    thr = a["threshold"][a["left"] >= 0]
    frac = (thr != thr.astype(np.float32)).mean()
    assert 0.05 < frac < 0.15
    leaf = (a["left"] < 0).reshape(nt, -1)
    vals = a["value1"].reshape(nt, -1)
    for t in range(nt):
        assert len(np.unique(vals[t][leaf[t]])) == leaf[t].sum()


def test_edge_rows_cover_the_edges(case):
    counts, U, E, seg = case["counts"], case["thresholds"], case["edge"], case["tables"]["seg"]
    X = E["X"]
    assert 4096 <= len(X) <= 20000 and X.shape[1] == 15
    assert (X == X.astype(np.float32)).sum() + np.isnan(X).sum() == X.size  # float32 values: no scaler rounding
    for f in range(15):
        c = counts[f]
        ks = set(E["pair_k"][E["pair_feature"] == f].tolist())
        if c == 0:
            assert not ks
            continue
        ns = -(-c // seg)
        want = {0, min(1, c - 1), c - 2, c - 1}
        if ns > 1:  # both sides of the first and of the last segment boundary
            want |= {seg - 1, seg, (ns - 1) * seg - 1, (ns - 1) * seg}
        want |= {k for j in range(1, c // SLOT_SPAN + 1) for k in (j * SLOT_SPAN - 1, j * SLOT_SPAN, j * SLOT_SPAN + 1)}
        if f in SEARCHED:
            want |= {3, 4}
        assert {k for k in want if 0 <= k < c} <= ks, f
        # the three rows of a k: at U[k], the float32 neighbours; ranks k, k or k - 1, k + 1
        at, above = E["pairs"][E["pair_feature"] == f].T
        k = E["pair_k"][E["pair_feature"] == f]
        np.testing.assert_array_equal(X[at, f], U[f][k])
        np.testing.assert_array_equal(np.searchsorted(U[f], X[at, f].astype(np.float32)), k)
        np.testing.assert_array_equal(np.searchsorted(U[f], X[above, f].astype(np.float32)), k + 1)
        np.testing.assert_array_equal(np.delete(X[at], f, axis=1), np.delete(X[above], f, axis=1))
        col = X[:, f]
        assert np.isposinf(col).any() and np.isneginf(col).any() and (np.isnan(col) & np.signbit(col)).any()
        assert (np.isnan(col) & ~np.signbit(col)).any() and (col == np.finfo(np.float32).max).any()
        if (U[f] == 0).any():
            assert ((col == 0) & np.signbit(col)).any() and ((col == 0) & ~np.signbit(col)).any()
    if max(counts) >= SLOT_SPAN:  # ranks 32,766 .. 32,768 are all there
        f = int(np.argmax(counts))
        r = np.searchsorted(U[f], X[:, f][~np.isnan(X[:, f])].astype(np.float32))
        assert {SLOT_SPAN - 1, SLOT_SPAN} <= set(r.tolist()) and (counts[f] == SLOT_SPAN or SLOT_SPAN + 1 in r)


def test_every_edge_pair_is_discriminating(case):
    """The oracle gives the rows (at U[k], just above U[k]) of every pair different probabilities:
    a condition on the generator and its seeds, not a measurement."""
    E = case["edge"]
    p = oracle.forest_predict(E["X"], case["arrays"])
    at, above = E["pairs"].T
    same = np.flatnonzero(p[at] == p[above])
    assert same.size == 0, (E["pair_feature"][same], E["pair_k"][same])


def test_fused_table_reaches_the_table_edges(case):
    """The synthetic table of the fused step: its amounts are float32 values, and the ranks of
    every searched feature's column reach rank 0 or the first segment, the last segment, and the
    last count of one segment with the first of the next."""
    d, X, seg = case["data"], case["table"], case["tables"]["seg"]
    assert 4096 <= len(X) <= 20000
    np.testing.assert_array_equal(d["amount"], d["amount"].astype(np.float32))
    for f in SEARCHED:
        u = case["thresholds"][f]
        if len(u) == 0:
            continue
        first, last, boundary = table_edge_report(X[:, f], u, seg)
        assert first and last and (boundary or len(u) <= seg), (f, first, last, boundary)


def test_edge_ranks_and_small_forest():
    rng = np.random.default_rng(0)
    assert edge_ranks(1, 16, True, rng) == [0]
    ks = edge_ranks(70000, 32, False, rng)
    assert {0, 1, 31, 32, 32766, 32767, 32768, 65533, 65534, 65535, 69998, 69999} <= set(ks)
    a, U = threshold_forest([3, 0, 5000], 4, rng)  # 15 internal nodes per tree
    assert [len(u) for u in U] == [3, 0, 5000] and len(a["node_offsets"]) - 1 == 1 + 334 + 2
    internal = a["left"] >= 0
    assert set(a["feature"][internal].tolist()) == {0, 2} and (a["feature"][~internal] == -2).all()
