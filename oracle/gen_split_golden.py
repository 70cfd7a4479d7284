"""Golden vectors for SURVEY §8(f) row f-4 (TEST INFRASTRUCTURE ONLY; build container only):
runs the reference's OWN get_train_test_set (shared_functions.py:133-188) and
card_precision_top_k (shared_functions.py:352-411), exec'd from shared_functions.py by
oracle/refexec.py, on the committed golden frame tests/golden/tiny_a.npz, and writes the
results to tests/golden/split_cpk.npz:

  train_ids / test_ids          TRANSACTION_IDs of get_train_test_set(df, start, 7, 7, 7)
  for start in three dates: train_ids_<k>, test_ids_<k>, start_ns_<k>
  cpk inputs: pred (float64, distinct values: no tie at any top-k boundary), day, customer,
  fraud; outputs nb_comp_<k>, cp_<k>, mean_<k> for top_k in (5, 20) with and without the
  removal of detected cards.

A second fixture, tests/golden/split_cpk_edges.npz, holds the same two reference functions on
tests/aux_ref.py's edge_frame (sparse and negative customer ids over more than three 256-thread
blocks, removed days, day numbering from 100, hot customers) -- see edges() below:

  inputs in narrow dtypes: ts_s (uint32 seconds after base_ns), day (int16), cust_idx (uint16
  index into cust_ids int32), fraud (uint8), pred (float32: the grid values are exact in it)
  split_<k>: split_start_ns_<k>, split_deltas_<k> (train, delay, test), split_sampling_<k>
  (ratio, random_state), train_ids_<k>, test_ids_<k> (int32)
  cpk_<k>: cpk_topk_<k>, cpk_remove_<k>, nb_comp_<k>, cp_<k>, mean_<k>

The Card-Precision predictions are tie-heavy; the generator asserts that no stored day is
tie-sensitive (aux_ref.card_precision), i.e. that the reference's result does not depend on
pandas' order among equal predictions, and that ties do straddle the cut on at least half of
the days of every case whose top_k is below the number of customers.

usage: python oracle/gen_split_golden.py
"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frame():
    z = np.load(os.path.join(ROOT, "tests", "golden", "tiny_a.npz"))
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")
    df = pd.DataFrame({k: z[k][o] for k in z.files})
    df["TX_DATETIME"] = df["TX_DATETIME"].astype("datetime64[ns]")
    start = np.datetime64("2024-06-01T00:00:00", "ns")
    df["TX_TIME_DAYS"] = ((df["TX_DATETIME"].values - start) // np.timedelta64(1, "D")).astype(np.int64)
    return df.reset_index(drop=True)


def main():
    import refexec

    ns = refexec.load_namespace()
    for fname in ("get_train_test_set", "card_precision_top_k_day", "card_precision_top_k"):
        exec(compile(refexec._shared_function_src(fname), f"<ref:shared_functions.py:{fname}>", "exec"), ns)
    df = frame()
    out = {}
    starts = [pd.Timestamp("2024-06-08"), pd.Timestamp("2024-06-20"), pd.Timestamp("2024-07-03")]
    for k, st in enumerate(starts):
        tr, te = ns["get_train_test_set"](df, st, delta_train=7, delta_delay=7, delta_test=7)
        out[f"train_ids_{k}"] = tr.TRANSACTION_ID.values.astype(np.int64)
        out[f"test_ids_{k}"] = te.TRANSACTION_ID.values.astype(np.int64)
        out[f"start_ns_{k}"] = np.int64(st.value)
    rng = np.random.default_rng(5)
    pred = rng.random(len(df))
    pred[df.TX_FRAUD.values == 1] += 0.3                      # a useful detector
    out["pred"] = pred
    pdf = df[["TX_TIME_DAYS", "CUSTOMER_ID", "TX_FRAUD"]].copy()
    pdf["predictions"] = pred
    k = 0
    for top_k in (5, 20):
        for rem in (True, False):
            nb, cp, mean = ns["card_precision_top_k"](pdf, top_k, remove_detected_compromised_cards=rem)
            out[f"cpk_topk_{k}"] = np.int64(top_k)
            out[f"cpk_remove_{k}"] = np.int64(rem)
            out[f"nb_comp_{k}"] = np.asarray(nb, np.int64)
            out[f"cp_{k}"] = np.asarray(cp, np.float64)
            out[f"mean_{k}"] = np.float64(mean)
            k += 1
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "split_cpk.npz"), **out)
    print({kk: (v.shape if hasattr(v, "shape") else v) for kk, v in out.items()})
    edges(ns)


# (start, delta_train, delta_delay, delta_test, sampling_ratio, random_state); calendar day
# index = days after 2024-06-01, days 16, 25 and 33 hold no rows (aux_ref.EDGE_REMOVED_DAYS)
EDGE_SPLITS = [
    ("2024-06-08", 7, 7, 7, 1.0, 0),          # day 16 is a delay day, day 25 a test day
    ("2024-06-03 10:30", 3, 0, 4, 1.0, 0),    # mid-day start, no delay: day 5 is train and test
    ("2024-06-20", 1, 1, 1, 1.0, 0),
    ("2024-06-25", 5, 2, 9, 1.0, 0),          # day 25 is a train day, day 33 a delay and a test day
    ("2024-06-15", 10, 7, 30, 1.0, 0),        # test days run past the end of the data
    ("2024-05-30", 7, 7, 7, 1.0, 0),          # starts before the first row: d0 is not the start's day
    ("2024-08-01", 7, 7, 7, 1.0, 0),          # starts after the last row: both sets empty
    ("2024-07-04", 7, 7, 7, 1.0, 0),          # starts on a removed day: d0 is the day after
    ("2024-06-08", 7, 7, 7, 0.5, 7),          # host-side subsampling of the train set
]
EDGE_TOPK = (1, 7, 100, 256, 257, 2000)


def edges(ns):
    import aux_ref

    f = aux_ref.edge_frame(aux_ref.EDGE_SEED)
    df = pd.DataFrame(f)
    df["TX_DATETIME"] = df["TX_DATETIME"].astype("datetime64[ns]")
    ids, cust_idx = np.unique(f["CUSTOMER_ID"], return_inverse=True)
    sec = (f["TX_DATETIME"] - aux_ref.EDGE_BASE_NS) // 10 ** 9
    pred = aux_ref.edge_predictions(f, aux_ref.EDGE_SEED, tie_safe=True)
    assert (pred == 0.0).any() and np.array_equal(pred.astype(np.float32).astype(np.float64), pred)
    assert len(ids) > 3 * 256 and ids.min() < 0
    out = {
        "seed": np.int64(aux_ref.EDGE_SEED), "base_ns": np.int64(aux_ref.EDGE_BASE_NS),
        "txid0": np.int64(f["TRANSACTION_ID"][0]),
        "ts_s": sec.astype(np.uint32), "day": f["TX_TIME_DAYS"].astype(np.int16),
        "cust_idx": cust_idx.astype(np.uint16), "cust_ids": ids.astype(np.int32),
        "fraud": f["TX_FRAUD"].astype(np.uint8), "pred": pred.astype(np.float32),
    }
    for k, (start, dtr, dde, dte, ratio, rs) in enumerate(EDGE_SPLITS):
        st = pd.Timestamp(start)
        tr, te = ns["get_train_test_set"](df, st, delta_train=dtr, delta_delay=dde, delta_test=dte,
                                          sampling_ratio=ratio, random_state=rs)
        out[f"split_start_ns_{k}"] = np.int64(st.value)
        out[f"split_deltas_{k}"] = np.array([dtr, dde, dte], np.int32)
        out[f"split_sampling_{k}"] = np.array([ratio, rs], np.float64)
        out[f"train_ids_{k}"] = tr.TRANSACTION_ID.values.astype(np.int32)
        out[f"test_ids_{k}"] = te.TRANSACTION_ID.values.astype(np.int32)
    pdf = df[["TX_TIME_DAYS", "CUSTOMER_ID", "TX_FRAUD"]].copy()
    pdf["predictions"] = pred
    cols = (f["TX_TIME_DAYS"], f["CUSTOMER_ID"], pred, f["TX_FRAUD"])
    k = 0
    for top_k in EDGE_TOPK:
        for rem in (True, False):
            sens = aux_ref.card_precision(*cols, top_k, rem)[3]
            assert not any(sens), f"top_k {top_k} remove {rem}: days {np.nonzero(sens)[0]} are tie-sensitive"
            tied = aux_ref.tied_at_cut(*cols, top_k, rem)
            if top_k < len(ids):  # a cut below the last customer exists at all
                assert 2 * sum(tied) >= len(tied), f"top_k {top_k} remove {rem}: ties straddle the cut on " \
                                                   f"{sum(tied)} of {len(tied)} days only"
            nb, cp, mean = ns["card_precision_top_k"](pdf, top_k, remove_detected_compromised_cards=rem)
            out[f"cpk_topk_{k}"] = np.int64(top_k)
            out[f"cpk_remove_{k}"] = np.int64(rem)
            out[f"nb_comp_{k}"] = np.asarray(nb, np.int16)
            out[f"cp_{k}"] = np.asarray(cp, np.float64)
            out[f"mean_{k}"] = np.float64(mean)
            k += 1
    path = os.path.join(ROOT, "tests", "golden", "split_cpk_edges.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "tiny_a.npz"))
    print(path, os.path.getsize(path), "bytes;", len(sec), "rows,", len(ids), "customers")


if __name__ == "__main__":
    main()
