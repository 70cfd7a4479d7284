"""The rank search tables at the sizes that shape them (forest_gen.RANK_CASES): 32- and 64-float
segments, sample tables filled to their last float and one threshold past it, every S-tree level
count and the step that drops the trees, 32,767 / 32,768 thresholds on one feature, v2 slot bases.

Every value of every scoring row is ranked by a two-level search (k_prepare, k_prepare_st,
k_prepare_v2) or an S-tree descent (k_prepare_st, k_zfill_grouped_w3) over tables whose shape
follows from the forest's threshold counts.  Each case first asserts through
fdx_forest_rank_tables / fdx_forest_layout that it is in the regime it names, then scores rows that
sit on the table edges (forest_gen.edge_rows: a threshold, the float32 below and above it, at
segment, sample, slot and table ends; test_forest_gen.py shows that every such pair scores
differently) under every kernel variant, and one fused pipeline step whose columns take the
thresholds' values.  The reference is the C oracle of sklearn's _apply_dense, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT
from forest_gen import (FUSED_CUSTOMERS, FUSED_TERMINALS, RANK_CASES, SEARCHED, SLOT_SPAN, expected_tables, rank_case,
                        table_edge_report)
from fdx import _lib, ops
from fdx._lib import FdxError, FdxUnsupported
from fdx.pipeline import FraudPipeline

pytestmark = pytest.mark.gpu


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def layout(f):
    lay, ns = ctypes.c_int32(), ctypes.c_int32()
    assert _lib.load().fdx_forest_layout(f._h, ctypes.byref(lay), ctypes.byref(ns)) == 0
    return lay.value, ns.value


def shape(f):
    t = f.rank_tables()
    return t["seg"], t["n_samples"], t["n_tree_floats"], t["tree_levels"]


@pytest.fixture(scope="module", params=list(RANK_CASES))
def case(request, dev):
    """One forest per case, shared by the tests below (each leaves it in its default variant);
    the oracle scores the edge rows and the fused step's table once."""
    c = rank_case(request.param)
    c["want"] = RANK_CASES[request.param][1]
    c["forest"] = ops.Forest(c["arrays"], 15)
    c["default"] = c["forest"].variant
    c["p_edge"] = oracle.forest_predict(c["edge"]["X"], c["arrays"])
    c["p_table"] = oracle.forest_predict(c["table"], c["arrays"])
    return c


def slots_v2(counts):
    return sum(max(1, -(-n // SLOT_SPAN)) for n in counts)


def test_case_is_in_its_regime(case):
    f, counts, want = case["forest"], case["counts"], case["want"]
    assert shape(f) == want
    assert want == (case["tables"]["seg"], case["tables"]["n_samples"], case["tables"]["n_tree_floats"],
                    case["tables"]["tree_levels"])
    if case["v2"]:  # a feature past 32,767 thresholds: v2 rows, paired planes (every tree fits below the slots)
        assert layout(f) == (2, slots_v2(counts)) and f.variant == 5
    else:           # v3 borrow nodes over v1 rows
        assert layout(f) == (1, 15) and f.variant == 6
    name = case["name"]
    if name in ("v1_full", "v1_full_no_trees"):
        assert want[:2] == (16, 8192)      # s_smp[kMaxRankSamples] is full
    if name == "v2_full":
        assert want[:2] == (16, 20480) and layout(f) == (2, 25)  # k_prepare_v2's table is full; 5 x 3 + 10 slots
    if name == "v2_first":
        assert layout(f) == (2, 16)
    if name in ("v1_one_more", "v2_one_more"):
        assert want[0] == 32
    if name.startswith("seg64"):
        assert want[0] == 64


def test_edge_rows_under_every_variant(case, dev):
    """Forest.predict of the edge rows == the oracle under every variant the forest accepts; the
    refused ones say why and leave the tables as they were.  A forest that fits v1 keeps its v1
    table shape under the v2-node variants 2-5 (one slot per feature, v1 rows: the 8,192-sample
    table of the v1-row kernels, not k_prepare_v2's 20,480)."""
    f, want = case["forest"], case["want"]
    X = T(case["edge"]["X"], torch.float64, dev)
    refusals = {1: "needs rank layout v1, which this forest does not fit",
                6: "needs rank layout v3, which this forest does not fit",
                3: "needs one threshold slot per feature"} if case["v2"] else {}
    for v in [case["default"]] + list(range(7)) + [case["default"]]:
        if v in refusals:
            before = (f.variant, layout(f), shape(f))
            with pytest.raises(FdxUnsupported, match=refusals[v]):
                f.set_variant(v)
            assert (f.variant, layout(f), shape(f)) == before
        else:
            f.set_variant(v)
            if v == 0:
                pass  # the wide layout: float32 rows, no rank tables read
            elif case["v2"]:
                assert layout(f) == (2, slots_v2(case["counts"])) and shape(f) == want
            else:
                assert layout(f) == {1: (1, 16), 6: (1, 15)}.get(v, (3, 15))
                assert shape(f) == want
        got = f.predict(X).cpu().numpy()
        bad = np.flatnonzero(got != case["p_edge"])
        assert bad.size == 0, (v, bad[:10], case["edge"]["X"][bad[:3]])
    assert f.variant == case["default"]


def test_fused_step(case, dev):
    """One run_fused step (3 windows) over a table whose amounts are feature 0's edge values and
    whose other columns take their features' threshold values: equal to pipe.run and to the oracle
    on the oracle's own feature table, under the default variant and under variant 3 (v2 nodes over
    v1 rows).  With S-trees the rows come from k_zfill_grouped_w3, without from k_zfill_grouped<16,
    true>.  A forest with v2 rows is refused by the fused assembly, by name."""
    f, d, table = case["forest"], case["data"], case["table"]
    seg = case["want"][0]
    for s in SEARCHED:  # (asserted on the host too: test_forest_gen.py)
        u = case["thresholds"][s]
        if len(u):
            first, last, boundary = table_edge_report(table[:, s], u, seg)
            assert first and last and (boundary or len(u) <= seg)
    n = len(d["ts"])
    args = (T(d["ts"], torch.int64, dev), T(d["customer"], torch.int32, dev), T(d["terminal"], torch.int32, dev),
            T(d["amount"], torch.float64, dev), T(d["fraud"], torch.uint8, dev), FUSED_CUSTOMERS, FUSED_TERMINALS)
    pipe = FraudPipeline(forest=f)
    assert len(pipe.windows_days) == 3
    feats, p_ref = pipe.run(*args)
    np.testing.assert_array_equal(feats.X.cpu().numpy(), table)
    np.testing.assert_array_equal(p_ref.cpu().numpy(), case["p_table"])
    if case["v2"]:
        with pytest.raises(FdxError, match="the fused scoring rows need the v1 row format"):
            pipe.run_fused(*args, torch.empty(n, dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
        return
    for v in (case["default"], 3, case["default"]):
        f.set_variant(v)
        assert shape(f) == case["want"]
        p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        pipe.run_fused(*args, p, ops.workspace(f.workspace_size(n * 11 // 10), dev))
        got = p.cpu().numpy()
        bad = np.flatnonzero(got != case["p_table"])
        assert bad.size == 0, (v, bad[:10], table[bad[:3]])


def test_rank_tables_of_the_bench_model(dev):
    """fdx_forest_rank_tables on the benchmark's forest: 16-float segments, 5,040 samples, four
    4-level S-trees of 6,560 floats; null arguments are refused.  The sample count is the model's
    own: its thresholds, rounded down to float32 and counted per feature here with numpy (80,516
    distinct, at most 19,710 on one feature), one sample per 16 of a feature's."""
    z = np.load(os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    arrays = {k: z[k] for k in ("node_offsets", "left", "right", "feature", "threshold", "missing_left", "value1")}
    thr, feat = z["threshold"][z["left"] >= 0], z["feature"][z["left"] >= 0]
    t32 = thr.astype(np.float32)
    t32 = np.where(t32.astype(np.float64) > thr, np.nextafter(t32, np.float32(-np.inf)), t32)  # largest float32 <= thr
    counts = [len(np.unique(t32[feat == k])) for k in range(15)]
    assert sum(counts) == 80516 and max(counts) == 19710
    assert expected_tables(counts) == dict(seg=16, n_samples=5040, n_tree_floats=26240, tree_levels=[4, 4, 4, 4])
    f = ops.Forest(arrays, 15, z["mean"], z["scale"])
    assert f.rank_tables() == dict(seg=16, n_samples=5040, n_tree_floats=26240, tree_levels=[4, 4, 4, 4])
    f.set_variant(0)  # the wide kernel: the rank layout stays installed
    assert shape(f) == (16, 5040, 26240, [4, 4, 4, 4])
    L = _lib.load()
    seg = ctypes.c_int32()
    assert L.fdx_forest_rank_tables(f._h, ctypes.byref(seg), None, None, None) == -1
    assert b"null" in L.fdx_last_error()
    wide = ops.Forest(dict(arrays, feature=np.where(z["feature"] >= 0, z["feature"] + 5, z["feature"])), 20)
    assert layout(wide)[0] == 0 and shape(wide) == (0, 0, 0, [0, 0, 0, 0])  # > 15 features: no rank layout
