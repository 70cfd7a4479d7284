"""Drop-in replacements for the reference's featurization functions (pandas contract).

Same names, arguments, column names, dtypes and row/index layout as
fraud_detection_model/feature_transformation.ipynb:

  is_weekend(tx_datetime)                                        :246-253
  is_night(tx_datetime)                                          :294-301
  get_customer_spending_behaviour_features(customer_transactions,
                                           windows_size_in_days=[1,7,30])   :601-628
  get_count_risk_rolling_window(terminal_transactions, delay_period=7,
                                windows_size_in_days=[1,7,30],
                                feature="TERMINAL_ID")                       :1495-1522

Differences that make them a faster drop-in, not a different contract:
  * the per-group functions accept a frame holding MANY groups and process all of them in
    one GPU launch (``get_customer_spending_behaviour_features(df)`` returns exactly what
    ``df.groupby('CUSTOMER_ID').apply(lambda x: f(x))`` yields, rows grouped by key in key
    order, time order inside, index = TRANSACTION_ID); a single-group frame behaves like
    the reference per-group call;
  * is_weekend / is_night also accept a whole Series / array (one launch).
All arithmetic runs in libfdx.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import pandas as pd
import torch

from . import _lib, ops


def _to_dev(a: np.ndarray, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _ts_ns(values) -> np.ndarray:
    return np.asarray(values).astype("datetime64[ns]").astype(np.int64)


def _flags(tx_datetime, mode):
    dev = ops.require_gpu()
    scalar = isinstance(tx_datetime, (pd.Timestamp, np.datetime64)) or np.isscalar(tx_datetime)
    arr = _ts_ns([tx_datetime] if scalar else tx_datetime)
    we, ni = ops.time_flags(_to_dev(arr, torch.int64, dev), mode)
    return scalar, we.cpu().numpy().astype(np.int64), ni.cpu().numpy().astype(np.int64)


def is_weekend(tx_datetime, mode: int = _lib.FDX_FLAGS_NOTEBOOK):
    """int(weekday() >= 5) for a Timestamp, or an int64 array for a Series/array."""
    scalar, we, _ = _flags(tx_datetime, mode)
    if scalar:
        return int(we[0])
    return pd.Series(we, index=tx_datetime.index) if isinstance(tx_datetime, pd.Series) else we


def is_night(tx_datetime, mode: int = _lib.FDX_FLAGS_NOTEBOOK):
    """int(hour <= 6) for a Timestamp, or an int64 array for a Series/array."""
    scalar, _, ni = _flags(tx_datetime, mode)
    if scalar:
        return int(ni[0])
    return pd.Series(ni, index=tx_datetime.index) if isinstance(tx_datetime, pd.Series) else ni


def _dense_keys(keys: np.ndarray, dev):
    """Map arbitrary integer ids to dense int32 ids on the GPU, preserving key order."""
    k = torch.from_numpy(np.ascontiguousarray(keys.astype(np.int64))).to(dev)
    if len(keys) and keys.min() >= 0 and keys.max() < (1 << 24):
        return k.to(torch.int32), int(keys.max()) + 1
    ids, n_unique = ops.dense_ids_i64(k)  # sort-based dense re-id on the GPU (fdx_dense_ids_i64)
    return ids, int(n_unique.item())


def _grouped_order(df: pd.DataFrame, key_col: str, dev):
    """GPU grouping of the frame's rows by key, time order inside each key.
    Returns (order: np.ndarray row positions in grouped order, ts_d, perm_d, seg_d)."""
    ts = _ts_ns(df["TX_DATETIME"].values)
    ts_d = _to_dev(ts, torch.int64, dev)
    keys_d, n_keys = _dense_keys(df[key_col].values, dev)
    if not ops.is_sorted_i64(ts_d):
        tperm = ops.argsort_i64(ts_d)       # stable: ties keep frame order
        kp, seg, _ = ops.rekey(ops.gather(keys_d, tperm), n_keys)
        perm = ops.gather(tperm, kp)
    else:
        perm, seg, _ = ops.rekey(keys_d, n_keys)
    return perm, seg, ts_d


def _frame_out(df, perm_np, cols: dict, index_name="TRANSACTION_ID"):
    out = df.iloc[perm_np].copy()
    for name, vals in cols.items():
        out[name] = vals
    out.index = out[index_name].values
    out.index.name = index_name
    return out


def _empty_out(df, names, index_name="TRANSACTION_ID"):
    out = df.copy()
    for name in names:
        out[name] = np.zeros(0, np.float64)
    if index_name in out.columns:
        out.index = out[index_name].values
        out.index.name = index_name
    return out


def get_customer_spending_behaviour_features(customer_transactions: pd.DataFrame,
                                             windows_size_in_days: Sequence[int] = (1, 7, 30),
                                             mode: str = "exact"):
    """feature_transformation.ipynb:601-628 for one or many customers at once.  mode="exact":
    pandas' roll_sum bit for bit, for any float64 amount -- NaN is left out of count and sum, +-inf
    is counted and left out of the sum, as pandas' rolling count() and sum() do; mode="scan":
    float64 prefix sums (counts exact, averages within ~1e-13 relative), which
    an infinite amount would poison for the rest of its segment: ValueError."""
    if mode not in ("exact", "scan"):
        raise ValueError("mode must be 'exact' or 'scan'")
    dev = ops.require_gpu()
    df = customer_transactions
    if len(df) == 0:  # pandas' groupby.apply of an empty frame: no rows, the new columns
        return _empty_out(df, [f"CUSTOMER_ID_{k}_{w}DAY_WINDOW" for w in windows_size_in_days
                               for k in ("NB_TX", "AVG_AMOUNT")])
    amt = df["TX_AMOUNT"].values.astype(np.float64)
    # (this function alone refuses: ops.customer_windows_scan and FraudPipeline(avg_mode="scan") take
    # finite or NaN amounts by contract, include/fdx.h, and do not look)
    if mode == "scan" and np.isinf(amt).any():
        raise ValueError("mode='scan' does not take infinite amounts (mode='exact' follows pandas on them)")
    perm, seg, ts_d = _grouped_order(df, "CUSTOMER_ID", dev)
    amt_d = _to_dev(amt, torch.float64, dev)
    if mode == "scan":
        nb, avg = ops.customer_windows_scan(ops.gather(ts_d, perm), ops.gather(amt_d, perm), seg,
                                            windows_size_in_days)
    else:
        nb, avg = ops.customer_windows(ops.gather(ts_d, perm), ops.gather(amt_d, perm), seg, windows_size_in_days)
    nb, avg, perm_np = nb.cpu().numpy(), avg.cpu().numpy(), perm.cpu().numpy()
    cols = {}
    for k, w in enumerate(windows_size_in_days):
        cols[f"CUSTOMER_ID_NB_TX_{w}DAY_WINDOW"] = nb[k].astype(np.float64)
        cols[f"CUSTOMER_ID_AVG_AMOUNT_{w}DAY_WINDOW"] = avg[k]
    return _frame_out(df, perm_np, cols)


def get_count_risk_rolling_window(terminal_transactions: pd.DataFrame, delay_period: int = 7,
                                  windows_size_in_days: Sequence[int] = (1, 7, 30),
                                  feature: str = "TERMINAL_ID"):
    """feature_transformation.ipynb:1495-1522 for one or many keys of `feature` at once."""
    dev = ops.require_gpu()
    df = terminal_transactions
    if len(df) == 0:
        return _empty_out(df, [f"{feature}_{k}_{w}DAY_WINDOW" for w in windows_size_in_days for k in ("NB_TX", "RISK")])
    perm, seg, ts_d = _grouped_order(df, feature, dev)
    fr_d = _to_dev((df["TX_FRAUD"].values != 0).astype(np.uint8), torch.uint8, dev)
    nb, risk = ops.terminal_windows(ops.gather(ts_d, perm), ops.gather(fr_d, perm), seg, delay_period,
                                    windows_size_in_days)
    nb, risk, perm_np = nb.cpu().numpy(), risk.cpu().numpy(), perm.cpu().numpy()
    cols = {}
    for k, w in enumerate(windows_size_in_days):
        cols[f"{feature}_NB_TX_{w}DAY_WINDOW"] = nb[k].astype(np.float64)
        cols[f"{feature}_RISK_{w}DAY_WINDOW"] = risk[k]
    out = _frame_out(df, perm_np, cols)
    # the reference ends with terminal_transactions.fillna(0, inplace=True) (:1520)
    out.fillna(0, inplace=True)
    return out
