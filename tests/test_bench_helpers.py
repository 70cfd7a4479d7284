"""Host-side helpers of bench.py (no GPU): the forest's walk-step count used by the LDS
roofline."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_walk_steps_per_row_sums_tree_depths():
    b = _bench()
    # tree 0: root -> (leaf, node -> (leaf, leaf)): depth 2; tree 1: a single leaf: depth 0;
    # tree 2: root -> (leaf, leaf): depth 1   (pre-order, -1 = leaf, per-tree local ids)
    left = np.array([1, -1, 3, -1, -1, -1, 1, -1, -1])
    right = np.array([2, -1, 4, -1, -1, -1, 2, -1, -1])
    off = np.array([0, 5, 6, 9])
    assert b.walk_steps_per_row({"left": left, "right": right, "node_offsets": off}) == 3


def test_walk_steps_of_the_bench_model():
    b = _bench()
    z = np.load(os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    a = {k: z[k] for k in ("left", "right", "node_offsets")}
    assert b.walk_steps_per_row(a) == 2000  # 100 trees, every one reaches depth 20
    assert b.LDS_PEAK_STEPS == 256 * 2.4e9 / 4 * 64


def test_sklearn_forest_rebuilt_from_arrays_matches_saved_output():
    """The CPU baseline times scikit-learn itself on the bench model, rebuilt from its node
    arrays (no pickle): the rebuilt forest must give sklearn's saved predict_proba bit for bit."""
    import sklearn.preprocessing

    b = _bench()
    arrays, mean, scale, cx, cp = b.load_model(os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    rf = b.sklearn_forest(arrays)
    sc = sklearn.preprocessing.StandardScaler()
    sc.mean_, sc.scale_, sc.var_, sc.n_features_in_, sc.n_samples_seen_ = mean, scale, scale * scale, 15, 1
    rf.set_params(n_jobs=1)
    np.testing.assert_array_equal(rf.predict_proba(sc.transform(cx[:512]))[:, 1], cp[:512])


def test_host_info_fields():
    info = _bench().host_info()
    assert info["nproc"] >= 1 and info["affinity_cpus"] >= 1 and info["joblib_cpus"] >= 1


def test_plan_workload_configs1_at_one_gpu():
    b = _bench()
    w = b.plan_workload(1, 0)
    assert w["name"] == "configs1" and w["scaling"] == "weak"
    assert (w["customer_base"], w["n_customers_local"], w["n_terminals_total"], w["days"]) == (0, 50_000, 100_000, 183)


def test_plan_workload_configs3_strong_scaling_over_8_ranks():
    """bench.py --gpus 8 runs BASELINE.json configs[3]: 1M customers / 2M terminals / 365 days in
    total, contiguous customer ranges, the terminal id space independent of N."""
    b = _bench()
    for world in (2, 4, 8):
        plans = [b.plan_workload(world, r) for r in range(world)]
        assert all(p["name"] == "configs3" and p["scaling"] == "strong" for p in plans)
        assert all(p["n_terminals_total"] == 2_000_000 and p["days"] == 365 for p in plans)
        assert plans[0]["customer_base"] == 0
        for a, c in zip(plans, plans[1:]):
            assert a["customer_base"] + a["n_customers_local"] == c["customer_base"]
        assert sum(p["n_customers_local"] for p in plans) == 1_000_000
    p8 = [b.plan_workload(8, r) for r in range(8)]
    assert [(p["customer_base"], p["n_customers_local"]) for p in p8] == [(r * 125_000, 125_000) for r in range(8)]


def test_stage_table_medians_and_rejects_inflated_isolated_times():
    """An isolated stage time more than 2x its in-step time (BENCH_r03: one cold step of 15-21 ms
    folded into a mean of 3) is rejected: the roofline uses the in-step median instead."""
    b = _bench()
    stages = [("rekey_customer", "K2", []), ("customer_walk", "K1-cust", []), ("forest_traverse", "K3", [])]
    in_step = {"rekey_customer": [0.9, 0.95, 1.0], "customer_walk": [1.0, 1.0, 1.1], "forest_traverse": [7.2, 7.1, 7.3]}
    iso = {"rekey_customer": [0.58, 15.9, 0.59], "customer_walk": [21.0, 22.0, 0.75], "forest_traverse": [7.0, 7.1, 7.2]}
    rows = {r["stage"]: r for r in b.stage_table(in_step, iso, stages)}
    assert rows["rekey_customer"]["ms"] == 0.59 and rows["rekey_customer"]["ms_isolated"] == 0.59  # median
    assert "ms_isolated" not in rows["customer_walk"]
    assert rows["customer_walk"]["ms_isolated_rejected"] == 21.0
    assert rows["customer_walk"]["ms"] == rows["customer_walk"]["ms_in_step"] == 1.0
    assert rows["forest_traverse"]["ms"] == 7.1
    assert b.stage_table(in_step, None, stages)[0]["ms"] == 0.95


def test_full_gates_the_extra_legs():
    """A plain run is the timed steps only; --sweep-variant belongs to --full, --steps counts
    timed steps (at least one)."""
    import pytest

    b = _bench()
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    assert b.parse(["--full", "--sweep-variant", "1,2", "--dump-outputs", "d"]).dump_outputs == "d"
    for bad in (["--sweep-variant", "1"], ["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            b.parse(bad)


def _filled_table(ops, n, slot_of_row, cap):
    """A FeatureTable (host memory) whose slot slot_of_row[r] holds row r with features f(r)."""
    import torch

    t = ops.FeatureTable(cap, torch.device("cpu"))
    t.buf.zero_()
    col = t.columns()
    col["row"].fill_(-1)
    s = torch.from_numpy(slot_of_row)
    r = torch.arange(n)
    col["row"][s] = r.int()
    for w in range(3):
        col["cust_nb"][w][s] = (r * 3 + w).int()
        col["term_nb"][w][s] = (r * 5 + w).int()
        col["cust_avg"][w][s] = r.double() + 0.25 * w
        col["term_risk"][w][s] = 1.0 / (r.double() + 1 + w)
    col["weekend"][s] = (r % 2).to(torch.uint8)
    col["night"][s] = (r % 3 == 0).to(torch.uint8)
    return t


def _want_features(rows):
    r = rows.astype(np.float64)
    cols = [rows % 2, rows % 3 == 0]
    for nb, val in ((lambda w: r * 3 + w, lambda w: r + 0.25 * w), (lambda w: r * 5 + w, lambda w: 1.0 / (r + 1 + w))):
        for w in range(3):
            cols += [nb(w), val(w)]
    return np.column_stack(cols).astype(np.float64)


def test_dump_outputs_reads_the_table_by_input_row(tmp_path):
    """--dump-outputs: float64 .npy files, rows ascending, proba and the 14 feature columns of those
    input rows whatever slot the table holds them in; the same seeded sample on every call."""
    import torch

    from fdx import ops

    b = _bench()
    n, cap = 1000, 1152
    slot_of_row = np.random.default_rng(5).permutation(1100)[:n]
    table = _filled_table(ops, n, slot_of_row, cap)
    proba = torch.arange(n, dtype=torch.float64) / n
    b.dump_outputs(str(tmp_path / "all"), proba, table, 1100)
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("rows", "proba", "features")}
    assert all(v.dtype == np.float64 for v in got.values())
    np.testing.assert_array_equal(got["rows"], np.arange(n))
    np.testing.assert_array_equal(got["proba"], proba.numpy())
    np.testing.assert_array_equal(got["features"], _want_features(np.arange(n)))
    b.DUMP_ROWS = 64  # a larger output: a fixed sample
    b.dump_outputs(str(tmp_path / "s1"), proba, table, 1100)
    b.dump_outputs(str(tmp_path / "s2"), proba, None, 0)
    rows = np.load(tmp_path / "s1" / "rows.npy")
    assert rows.shape == (64,) and (np.diff(rows) > 0).all() and rows.max() < n
    np.testing.assert_array_equal(rows, np.load(tmp_path / "s2" / "rows.npy"))
    assert not (tmp_path / "s2" / "features.npy").exists()
    np.testing.assert_array_equal(np.load(tmp_path / "s1" / "proba.npy"), rows / n)
    np.testing.assert_array_equal(np.load(tmp_path / "s1" / "features.npy"), _want_features(rows.astype(np.int64)))


def test_bench_stream_splits_configs4_state_over_ranks():
    """bench_stream.py --gpus N: the 1M / 2M-key state of configs[4] split over the ranks --
    contiguous customer ranges covering every id once, every rank with all terminal ids."""
    import bench_stream

    a = bench_stream.parse([])
    assert (a.customers, a.terminals, a.batch) == (1_000_000, 2_000_000, 65536)
    for world in (1, 2, 4, 8):
        shards = [bench_stream.rank_shard(a, world, r) for r in range(world)]
        covered = np.concatenate([np.arange(base, base + n_c) for n_c, base, _ in shards])
        np.testing.assert_array_equal(covered, np.arange(1_000_000))
        assert all(t == 2_000_000 for _, _, t in shards)
