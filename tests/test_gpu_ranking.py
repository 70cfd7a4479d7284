"""SURVEY.md §8(f) row f-5 on the GPU: fdx_ranking_metrics / fdx_threshold_counts (csrc/fdx_metrics.hip)
and their fdx.evaluation callers (performance_assessment, performance_assessment_model_collection,
threshold_based_metrics: shared_functions.py:442-489, :538-581) against the exact reference of
tests/ranking_ref.py and scikit-learn.

Integer fields, the curve and auc are compared exactly (auc = one IEEE division of operands
< 2^53 = Python's correctly rounded int / int).  ap is a float64 sum of non-negative terms: its
relative error is at most (chain + 3) * 2^-53, chain = the longest chain of additions behind one
term as stated next to k_group_reduce: ceil(m / (grid * 256)) + 8 + ceil(grid / 256) + 8 with
grid = min(ceil(n / 4096), 1024) blocks and m <= n groups, + 3 for the term's division and
product and the final / P.  For n <= 2^22 that is at most (36 + 3) * 2^-53 = 4.4e-15.
"""
import math
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import ranking_ref as rr
from fdx import FdxError, evaluation, ops

pytestmark = pytest.mark.gpu

THRESHOLDS = [0, 0.01, 0.5, 1.0, 1.01, -1, 0.5]  # unsorted, one duplicate, values equal to scores


def ap_tolerance(n):
    grid = min(max(-(-n // 4096), 1), 1024)
    chain = -(-n // (grid * 256)) + 8 + -(-grid // 256) + 8
    tol = (chain + 3) * 2.0 ** -53
    assert tol <= 1e-13
    return tol


def rel(a, ref):
    return abs(a - ref) / abs(ref) if ref else abs(a - ref)


def bits(r):
    return (r["n_pos"], r["n_neg"], r["n_groups"], r["n_nonfinite"], r["auc_num"], np.float64(r["auc"]).tobytes(),
            np.float64(r["ap"]).tobytes())


def to_dev(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the named inputs are read-only)


def run(dev, s, y, curve=False):
    return ops.ranking_metrics(to_dev(dev, s), to_dev(dev, y), curve=curve)


_results = {}


def result_of(dev, name):
    """One call with the curve per named input, shared by the tests below."""
    if name not in _results:
        rm = run(dev, *rr.named_inputs()[name], curve=True)
        _results[name] = (rm.host(), [t.cpu().numpy() for t in rm.curve()])
    return _results[name]


@pytest.mark.parametrize("name", rr.NAMES)
def test_ranking_metrics_match_the_exact_reference(dev, name):
    e = rr.exact_of(name)
    r, (fps, tps, thr) = result_of(dev, name)
    n = len(rr.named_inputs()[name][0])
    assert r["n_nonfinite"] == 0
    assert (r["n_pos"], r["n_neg"], r["n_groups"], r["auc_num"]) == (e["n_pos"], e["n_neg"], e["n_groups"], e["auc_num"])
    np.testing.assert_array_equal(thr, e["thr"])
    np.testing.assert_array_equal(tps, e["tps"])
    np.testing.assert_array_equal(fps, e["fps"])
    assert np.float64(r["auc"]).tobytes() == np.float64(e["auc"]).tobytes() or (math.isnan(r["auc"]) and
                                                                               math.isnan(e["auc"]))
    err = abs(Fraction(r["ap"]) - e["ap"])
    tol = ap_tolerance(n)
    print(name, "n", n, "groups", r["n_groups"], "ap rel err", float(err / e["ap"]) if e["ap"] else float(err),
          "tolerance", tol)
    assert err <= Fraction(tol) * e["ap"]
    if name == "empty":
        assert r["n_groups"] == 0 and math.isnan(r["auc"]) and r["ap"] == 0.0
    if name in ("no_pos", "no_neg"):
        assert math.isnan(r["auc"])


@pytest.mark.parametrize("name", [n for n in rr.NAMES if rr.both_classes(n)])
def test_ranking_metrics_match_sklearn(dev, name):
    r, _ = result_of(dev, name)
    auc, ap = rr.sklearn_of(name)
    print(name, "auc rel", rel(r["auc"], auc), "ap rel", rel(r["ap"], ap))
    assert rel(r["auc"], auc) <= 1e-12
    assert rel(r["ap"], ap) <= 1e-12


@pytest.mark.parametrize("name", rr.NAMES)
def test_result_is_bit_identical_between_calls_and_row_orders(dev, name):
    s, y = rr.named_inputs()[name]
    first = bits(result_of(dev, name)[0])
    assert bits(run(dev, s, y).host()) == first
    o = np.random.default_rng(7).permutation(len(s))
    assert bits(run(dev, s[o], y[o]).host()) == first


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_scores_are_counted_and_refused(dev, bad):
    s, y = rr.named_inputs()["ties100"]
    s = s.copy()
    s[[5, 4098]] = bad
    assert run(dev, s, y).host()["n_nonfinite"] == 2
    df = pd.DataFrame({"TX_FRAUD": y, "predictions": s, "TX_TIME_DAYS": 0, "CUSTOMER_ID": np.arange(len(s))})
    with pytest.raises(ValueError):
        evaluation.performance_assessment(df)


def counts_numpy(s, y, thresholds):
    """TN, FP, FN, TP per threshold: predicted 1 iff not (p < threshold)."""
    out = []
    pos = np.asarray(y) != 0
    for t in thresholds:
        with np.errstate(invalid="ignore"):
            one = ~(s < t)
        out.append([int((~one & ~pos).sum()), int((one & ~pos).sum()), int((~one & pos).sum()), int((one & pos).sum())])
    return np.array(out, np.int64)


def threshold_inputs(name):
    s, y = rr.named_inputs()[name]
    if name == "signs":  # one NaN score: predicted 1 at every threshold
        s, y = np.r_[s, np.nan], np.r_[y, np.uint8(1)]
    return s, y


@pytest.mark.parametrize("name", ["ties100", "signs"])
def test_threshold_counts(dev, name):
    s, y = threshold_inputs(name)
    thr = np.sort(np.array(THRESHOLDS, np.float64))
    got = ops.threshold_counts(to_dev(dev, s), to_dev(dev, y), to_dev(dev, thr)).cpu().numpy()
    np.testing.assert_array_equal(got, counts_numpy(s, y, thr))


def test_threshold_counts_limits(dev):
    s, y = threshold_inputs("ties100")
    sd, yd = to_dev(dev, s), to_dev(dev, y)
    thr = np.linspace(-0.1, 1.1, 1025)
    got = ops.threshold_counts(sd, yd, to_dev(dev, thr[:1024])).cpu().numpy()
    np.testing.assert_array_equal(got, counts_numpy(s, y, thr[:1024]))
    with pytest.raises(FdxError):
        ops.threshold_counts(sd, yd, to_dev(dev, thr))
    with pytest.raises(FdxError):
        ops.threshold_counts(sd, yd, torch.tensor([0.1, float("nan")], dtype=torch.float64, device=dev))
    with pytest.raises(FdxError):
        ops.threshold_counts(sd, yd, torch.tensor([0.5, 0.1], dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        evaluation.threshold_based_metrics(s, y, [0.1, float("nan")])


def metrics_row(threshold, TN, FP, FN, TP):
    """shared_functions.py:548-577 on numpy integers."""
    with np.errstate(divide="ignore", invalid="ignore"):
        MME = (FP + FN) / (TN + FP + FN + TP)
        TPR, TNR, FPR, FNR = TP / (TP + FN), TN / (TN + FP), FP / (TN + FP), FN / (TP + FN)
        BER = 1 / 2 * (FPR + FNR)
        Gmean = np.sqrt(TPR * TNR)
        precision, FDR = (TP / (TP + FP), FP / (TP + FP)) if TP + FP > 0 else (1, 1)
        NPV, FOR = (TN / (TN + FN), FN / (TN + FN)) if TN + FN > 0 else (1, 1)
        F1 = 2 * (precision * TPR) / (precision + TPR)
    return [threshold, MME, TPR, TNR, FPR, FNR, BER, Gmean, precision, NPV, FDR, FOR, F1]


@pytest.mark.parametrize("name", ["ties100", "signs"])
def test_threshold_based_metrics(dev, name):
    s, y = threshold_inputs(name)
    df = evaluation.threshold_based_metrics(s, y, THRESHOLDS)
    cols = ["Threshold", "MME", "TPR", "TNR", "FPR", "FNR", "BER", "G-mean", "Precision", "NPV", "FDR", "FOR",
            "F1 Score"]
    assert list(df.columns) == cols and len(df) == len(THRESHOLDS)
    exp = [metrics_row(t, *c) for t, c in zip(THRESHOLDS, counts_numpy(s, y, THRESHOLDS))]
    for j, c in enumerate(cols):
        np.testing.assert_array_equal(df[c].values.astype(np.float64), np.array([r[j] for r in exp], np.float64), c)
    if name == "ties100":  # nothing is predicted 1 at 1.01: the defaults of 1, and F1 = 2 * (1 * 0) / (1 + 0)
        row = df.iloc[THRESHOLDS.index(1.01)]
        assert row["Precision"] == 1 and row["FDR"] == 1 and row["TPR"] == 0 and row["F1 Score"] == 0


def _frame(golden):
    z = golden("tiny_a.npz")
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")
    df = pd.DataFrame({k: z[k][o] for k in z.files})
    df["TX_DATETIME"] = df["TX_DATETIME"].astype("datetime64[ns]")
    start = np.datetime64("2024-06-01T00:00:00", "ns")
    df["TX_TIME_DAYS"] = ((df["TX_DATETIME"].values - start) // np.timedelta64(1, "D")).astype(np.int64)
    return df.reset_index(drop=True)


def test_performance_assessment(dev, golden):
    from sklearn.metrics import average_precision_score, roc_auc_score

    g = golden("split_cpk.npz")
    df = _frame(golden)
    pdf = df[["TX_TIME_DAYS", "CUSTOMER_ID", "TX_FRAUD"]].copy()
    pdf["predictions"] = g["pred"]
    ks = [k for k in range(4) if int(g[f"cpk_remove_{k}"]) == 1]  # performance_assessment removes detected cards
    top_k_list = [int(g[f"cpk_topk_{k}"]) for k in ks]
    auc, ap = roc_auc_score(pdf.TX_FRAUD, pdf.predictions), average_precision_score(pdf.TX_FRAUD, pdf.predictions)
    expect = [round(auc, 3), round(ap, 3)] + [round(float(g[f"mean_{k}"]), 3) for k in ks]
    cols = ["AUC ROC", "Average precision"] + [f"Card Precision@{k}" for k in top_k_list]
    perf = evaluation.performance_assessment(pdf, top_k_list=top_k_list)
    assert list(perf.columns) == cols and len(perf) == 1
    assert perf.iloc[0].tolist() == expect
    raw = evaluation.performance_assessment(pdf, top_k_list=[], rounded=False)
    assert rel(raw["AUC ROC"][0], auc) <= 1e-12 and rel(raw["Average precision"][0], ap) <= 1e-12

    # two classifiers: the golden predictions, and their reverse ranking
    auc2, ap2 = roc_auc_score(pdf.TX_FRAUD, -g["pred"] + 2.0), average_precision_score(pdf.TX_FRAUD, -g["pred"] + 2.0)
    both = evaluation.performance_assessment_model_collection(
        {"forest": {"predictions_test": g["pred"]}, "reversed": {"predictions_test": -g["pred"] + 2.0}},
        pdf.drop(columns="predictions"), type_set="test", top_k_list=top_k_list)
    assert list(both.index) == ["forest", "reversed"] and list(both.columns) == cols
    assert both.loc["forest"].tolist() == expect
    assert both.loc["reversed"].tolist()[:2] == [round(auc2, 3), round(ap2, 3)]


def test_curve_points(dev):
    s, y = rr.named_inputs()["ties100"]
    e = rr.exact_of("ties100")
    for f in (evaluation.roc_curve_points, evaluation.pr_curve_points):
        fps, tps, thr = f(s, y)
        np.testing.assert_array_equal(fps, e["fps"])
        np.testing.assert_array_equal(tps, e["tps"])
        np.testing.assert_array_equal(thr, e["thr"])


def test_device_path_from_run_fused(dev, golden):
    """run_fused's device output and the fraud column go straight into ops.ranking_metrics."""
    from fdx.pipeline import FraudPipeline

    z = golden("tiny_b.npz")
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")
    c = {k: z[k][o] for k in z.files}
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(dev, d)  # noqa: E731
    fz = golden("forest_rf5d8.npz")
    arrays = {k: fz[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    pipe = FraudPipeline(forest=ops.Forest(arrays, 15, fz["mean"], fz["scale"]))
    fraud = t(c["TX_FRAUD"], torch.uint8)
    proba = torch.empty(len(c["TX_FRAUD"]), dtype=torch.float64, device=dev)
    pipe.run_fused(t(c["TX_DATETIME"], torch.int64), t(c["CUSTOMER_ID"], torch.int32), t(c["TERMINAL_ID"], torch.int32),
                   t(c["TX_AMOUNT"], torch.float64), fraud, int(c["CUSTOMER_ID"].max()) + 1,
                   int(c["TERMINAL_ID"].max()) + 1, proba)
    r = ops.ranking_metrics(proba, fraud).host()
    e = rr.exact(proba.cpu().numpy(), c["TX_FRAUD"])
    assert (r["n_pos"], r["n_neg"], r["n_groups"], r["auc_num"], r["n_nonfinite"]) == (
        e["n_pos"], e["n_neg"], e["n_groups"], e["auc_num"], 0)
    assert r["auc"] == e["auc"]
    assert abs(Fraction(r["ap"]) - e["ap"]) <= Fraction(ap_tolerance(len(c["TX_FRAUD"]))) * e["ap"]
