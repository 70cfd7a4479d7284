"""the delay-aware train/test split, Card-Precision@k and the
score ranking metrics, so that model-quality parity (model_training.ipynb:2329-2341: AUC ROC,
AP, CP@100) runs on the GPU outputs.  Same names, arguments and return shapes as the reference:

  get_train_test_set(transactions_df, start_date_training, delta_train=7, delta_delay=7,
                     delta_test=7, sampling_ratio=1.0, random_state=0)
                                                        shared_functions.py:133-188
  card_precision_top_k(predictions_df, top_k, remove_detected_compromised_cards=True)
                                                        shared_functions.py:384-411
  performance_assessment(predictions_df, output_feature='TX_FRAUD',
                         prediction_feature='predictions', top_k_list=[100], rounded=True)
                                                        shared_functions.py:442-460
  performance_assessment_model_collection(fitted_models_and_predictions_dictionary,
                                          transactions_df, type_set='test', top_k_list=[100])
                                                        shared_functions.py:470-489
  threshold_based_metrics(fraud_probabilities, true_label, thresholds_list)
                                                        shared_functions.py:538-581
plus roc_curve_points / pr_curve_points, the curve arrays behind the notebook's ROC and PR plots.
The row selection (split masks, per-day per-card maxima, top-k) runs in libfdx.so
(csrc/fdx_aux.hip), the ranking metrics and the threshold counts in csrc/fdx_metrics.hip
(ops.ranking_metrics / ops.threshold_counts take device tensors; the functions here take the
reference's host frames and copy them in).  sampling_ratio < 1 subsamples the train set with
pandas' own DataFrame.sample (the reference's RNG), on the host.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import torch

from . import _lib, ops
from ._lib import check
from .features import _dense_keys, _to_dev, _ts_ns


def get_train_test_set(transactions_df: pd.DataFrame, start_date_training, delta_train=7, delta_delay=7,
                       delta_test=7, sampling_ratio=1.0, random_state=0):
    dev = ops.require_gpu()
    df = transactions_df
    n = len(df)
    ts = _to_dev(_ts_ns(df["TX_DATETIME"].values), torch.int64, dev)
    day = _to_dev(df["TX_TIME_DAYS"].values.astype(np.int32), torch.int32, dev)
    cust, n_cust = _dense_keys(df["CUSTOMER_ID"].values, dev)
    fraud = _to_dev((df["TX_FRAUD"].values != 0).astype(np.uint8), torch.uint8, dev)
    t_lo = int(pd.Timestamp(start_date_training).value)
    t_hi = t_lo + int(delta_train) * ops.NS_PER_DAY
    train = torch.empty(n, dtype=torch.uint8, device=dev)
    test = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = ops.workspace(n_cust * 5 + 64, dev)
    dmin = ctypes.c_int32(0)
    check(_lib.load().fdx_train_test_split(ops._ptr(ts), ops._ptr(day), ops._ptr(cust), ops._ptr(fraud), n, n_cust,
                                           t_lo, t_hi, int(delta_train), int(delta_delay), int(delta_test),
                                           ops._ptr(train), ops._ptr(test), ops._ptr(ws), ws.numel(),
                                           ctypes.byref(dmin), ops._s()), "fdx_train_test_split")
    train_df = df[train.cpu().numpy().astype(bool)]
    test_df = df[test.cpu().numpy().astype(bool)]
    if sampling_ratio < 1:
        train_df_frauds = train_df[train_df.TX_FRAUD == 1].sample(frac=sampling_ratio, random_state=random_state)
        train_df_genuine = train_df[train_df.TX_FRAUD == 0].sample(frac=sampling_ratio, random_state=random_state)
        train_df = pd.concat([train_df_frauds, train_df_genuine])
    return train_df.sort_values("TRANSACTION_ID"), test_df.sort_values("TRANSACTION_ID")


def card_precision_top_k(predictions_df: pd.DataFrame, top_k: int, remove_detected_compromised_cards=True):
    """-> (nb_compromised_cards_per_day, card_precision_top_k_per_day_list, mean)."""
    dev = ops.require_gpu()
    df = predictions_df
    days = np.sort(df["TX_TIME_DAYS"].unique()).astype(np.int32)
    pred = df["predictions"].values.astype(np.float64)
    if len(pred) and (pred.min() < 0 or np.isnan(pred).any()):
        raise _lib.FdxUnsupported("predictions must be >= 0 and not NaN")
    day = _to_dev(df["TX_TIME_DAYS"].values.astype(np.int32), torch.int32, dev)
    cust, n_cust = _dense_keys(df["CUSTOMER_ID"].values, dev)
    fraud = _to_dev((df["TX_FRAUD"].values != 0).astype(np.uint8), torch.uint8, dev)
    L = _lib.load()
    ws = ops.workspace(L.fdx_card_precision_workspace_size(n_cust), dev)
    nb = np.zeros(len(days), np.int32)
    cp = np.zeros(len(days), np.float64)
    check(L.fdx_card_precision_top_k(ops._ptr(day), ops._ptr(cust), ops._ptr(_to_dev(pred, torch.float64, dev)),
                                     ops._ptr(fraud), len(df), n_cust, days.ctypes.data, len(days), int(top_k),
                                     int(bool(remove_detected_compromised_cards)), nb.ctypes.data, cp.ctypes.data,
                                     ops._ptr(ws), ws.numel(), ops._s()), "fdx_card_precision_top_k")
    return nb.tolist(), cp.tolist(), float(np.array(cp).mean())


def _ranking(scores, labels, curve=False):
    """ops.ranking_metrics on host arrays -> (RankingMetrics, its fields); ValueError on NaN / inf
    scores, as sklearn's check_array raises."""
    dev = ops.require_gpu()
    s = _to_dev(np.asarray(scores, dtype=np.float64), torch.float64, dev)
    y = _to_dev((np.asarray(labels) != 0).astype(np.uint8), torch.uint8, dev)
    rm = ops.ranking_metrics(s, y, curve=curve)
    r = rm.host()
    if r["n_nonfinite"]:
        raise ValueError(f"Input contains NaN or infinity ({r['n_nonfinite']} predictions).")
    return rm, r


def performance_assessment(predictions_df: pd.DataFrame, output_feature="TX_FRAUD", prediction_feature="predictions",
                           top_k_list=[100], rounded=True):
    """-> one-row DataFrame: AUC ROC, Average precision, Card Precision@k per k."""
    _, r = _ranking(predictions_df[prediction_feature].values, predictions_df[output_feature].values)
    performances = pd.DataFrame([[r["auc"], r["ap"]]], columns=["AUC ROC", "Average precision"])
    for top_k in top_k_list:
        _, _, mean_card_precision_top_k = card_precision_top_k(predictions_df, top_k)
        performances["Card Precision@" + str(top_k)] = mean_card_precision_top_k
    if rounded:
        performances = performances.round(3)
    return performances


def performance_assessment_model_collection(fitted_models_and_predictions_dictionary, transactions_df,
                                            type_set="test", top_k_list=[100]):
    """-> one row per classifier, indexed by name (the reference's DataFrame.append, gone from
    pandas 2, is pd.concat here).  Like the reference, writes the 'predictions' column of
    transactions_df."""
    rows = []
    for classifier_name, model_and_predictions in fitted_models_and_predictions_dictionary.items():
        predictions_df = transactions_df
        predictions_df["predictions"] = model_and_predictions["predictions_" + type_set]
        performances_model = performance_assessment(predictions_df, output_feature="TX_FRAUD",
                                                    prediction_feature="predictions", top_k_list=top_k_list)
        performances_model.index = [classifier_name]
        rows.append(performances_model)
    return pd.concat(rows) if rows else pd.DataFrame()


def threshold_based_metrics(fraud_probabilities, true_label, thresholds_list):
    """-> DataFrame, one row per threshold in list order: Threshold, MME, TPR, TNR, FPR, FNR, BER,
    G-mean, Precision, NPV, FDR, FOR, F1 Score, from the device's TN, FP, FN, TP with the
    reference's float expressions (numpy scalars: a zero denominator gives nan / inf as there)."""
    dev = ops.require_gpu()
    thr = np.asarray(list(thresholds_list), dtype=np.float64)
    if np.isnan(thr).any():
        raise ValueError("thresholds_list contains NaN")
    order = np.argsort(thr, kind="stable")
    s = _to_dev(np.asarray(fraud_probabilities, dtype=np.float64), torch.float64, dev)
    y = _to_dev((np.asarray(true_label) != 0).astype(np.uint8), torch.uint8, dev)
    sorted_counts = ops.threshold_counts(s, y, _to_dev(thr[order], torch.float64, dev)).cpu().numpy()
    counts = np.empty_like(sorted_counts)
    counts[order] = sorted_counts
    results = []
    for threshold, (TN, FP, FN, TP) in zip(thresholds_list, counts):
        with np.errstate(divide="ignore", invalid="ignore"):
            MME = (FP + FN) / (TN + FP + FN + TP)
            TPR = TP / (TP + FN)
            TNR = TN / (TN + FP)
            FPR = FP / (TN + FP)
            FNR = FN / (TP + FN)
            BER = 1 / 2 * (FPR + FNR)
            Gmean = np.sqrt(TPR * TNR)
            precision = 1  # 1 if TP+FP=0
            FDR = 1  # 1 if TP+FP=0
            if TP + FP > 0:
                precision = TP / (TP + FP)
                FDR = FP / (TP + FP)
            NPV = 1  # 1 if TN+FN=0
            FOR = 1  # 1 if TN+FN=0
            if TN + FN > 0:
                NPV = TN / (TN + FN)
                FOR = FN / (TN + FN)
            F1_score = 2 * (precision * TPR) / (precision + TPR)
        results.append([threshold, MME, TPR, TNR, FPR, FNR, BER, Gmean, precision, NPV, FDR, FOR, F1_score])
    return pd.DataFrame(results, columns=["Threshold", "MME", "TPR", "TNR", "FPR", "FNR", "BER", "G-mean", "Precision",
                                          "NPV", "FDR", "FOR", "F1 Score"])


def roc_curve_points(scores, labels):
    """-> (fps, tps, thresholds) numpy arrays, one point per distinct score, thresholds
    decreasing: sklearn's _binary_clf_curve (no drop_intermediate).  FPR = fps / fps[-1],
    TPR = tps / tps[-1] are the notebook's ROC plot."""
    rm, _ = _ranking(scores, labels, curve=True)
    fps, tps, thr = rm.curve()
    return fps.cpu().numpy(), tps.cpu().numpy(), thr.cpu().numpy()


def pr_curve_points(scores, labels):
    """-> (fps, tps, thresholds) as roc_curve_points.  precision = tps / (tps + fps),
    recall = tps / tps[-1] are the notebook's PR plot."""
    return roc_curve_points(scores, labels)
