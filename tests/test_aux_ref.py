"""tests/aux_ref.py, the plain references the GPU tests of csrc/fdx_aux.hip compare with, pinned
on the CPU: split_masks and card_precision reproduce the reference project's own
get_train_test_set / card_precision_top_k on every case of tests/golden/split_cpk.npz and
split_cpk_edges.npz (written by oracle/gen_split_golden.py, which runs those functions);
edge_frame / edge_predictions still produce the inputs stored there; the segment, decode and
dedup references are checked on vectors whose answers are spelled out here."""
import numpy as np
import pandas as pd
import pytest

import aux_ref

N_EDGE_SPLITS = 9
N_EDGE_CPK = 12


def _tiny_frame(golden):
    z = golden("tiny_a.npz")
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")
    ts = z["TX_DATETIME"][o].astype("datetime64[ns]").astype(np.int64)
    start = int(np.datetime64("2024-06-01T00:00:00", "ns").astype(np.int64))
    return {"TRANSACTION_ID": z["TRANSACTION_ID"][o].astype(np.int64), "TX_DATETIME": ts,
            "TX_TIME_DAYS": (ts - start) // aux_ref.NS_PER_DAY, "CUSTOMER_ID": z["CUSTOMER_ID"][o].astype(np.int64),
            "TX_FRAUD": z["TX_FRAUD"][o].astype(np.int64)}


def _split(f, t_lo, deltas):
    return aux_ref.split_masks(f["TX_DATETIME"], f["TX_TIME_DAYS"], f["CUSTOMER_ID"], f["TX_FRAUD"], t_lo, *deltas)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_split_masks_reproduce_reference_on_tiny_frame(golden, k):
    g = golden("split_cpk.npz")
    f = _tiny_frame(golden)
    train, test = _split(f, int(g[f"start_ns_{k}"]), (7, 7, 7))
    np.testing.assert_array_equal(f["TRANSACTION_ID"][train], g[f"train_ids_{k}"])
    np.testing.assert_array_equal(f["TRANSACTION_ID"][test], g[f"test_ids_{k}"])


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_card_precision_reproduces_reference_on_tiny_frame(golden, k):
    g = golden("split_cpk.npz")
    f = _tiny_frame(golden)
    nb, cp, mean, sens = aux_ref.card_precision(f["TX_TIME_DAYS"], f["CUSTOMER_ID"], g["pred"], f["TX_FRAUD"],
                                                int(g[f"cpk_topk_{k}"]), bool(g[f"cpk_remove_{k}"]))
    assert not any(sens)
    np.testing.assert_array_equal(np.array(nb), g[f"nb_comp_{k}"])
    np.testing.assert_array_equal(np.array(cp), g[f"cp_{k}"])
    assert mean == float(g[f"mean_{k}"])


@pytest.mark.parametrize("k", range(N_EDGE_SPLITS))
def test_split_masks_reproduce_reference_on_edge_frame(golden, k):
    g = golden("split_cpk_edges.npz")
    f, _ = aux_ref.fixture_frame(g)
    train, test = _split(f, int(g[f"split_start_ns_{k}"]), [int(d) for d in g[f"split_deltas_{k}"]])
    ratio, random_state = g[f"split_sampling_{k}"]
    train_ids = f["TRANSACTION_ID"][train]
    if ratio < 1:  # the reference's host-side subsampling: pandas' own sample, frauds then genuine
        t = pd.DataFrame({"TRANSACTION_ID": train_ids, "TX_FRAUD": f["TX_FRAUD"][train]})
        t = pd.concat([t[t.TX_FRAUD == 1].sample(frac=ratio, random_state=int(random_state)),
                       t[t.TX_FRAUD == 0].sample(frac=ratio, random_state=int(random_state))])
        train_ids = np.sort(t.TRANSACTION_ID.values)
    np.testing.assert_array_equal(train_ids, g[f"train_ids_{k}"])
    np.testing.assert_array_equal(f["TRANSACTION_ID"][test], g[f"test_ids_{k}"])


def test_edge_split_cases_cover_what_they_are_for(golden):
    """an empty result, a removed delay day and a d0 that is not the start's day are in the fixture"""
    g = golden("split_cpk_edges.npz")
    assert f"split_start_ns_{N_EDGE_SPLITS}" not in g.files and f"cpk_topk_{N_EDGE_CPK}" not in g.files
    assert len(g["train_ids_6"]) == 0 and len(g["test_ids_6"]) == 0
    f, _ = aux_ref.fixture_frame(g)
    day_of = dict(zip(f["TRANSACTION_ID"].tolist(), f["TX_TIME_DAYS"].tolist()))
    for k in (5, 7):
        start_day = (int(g[f"split_start_ns_{k}"]) - int(g["base_ns"])) // aux_ref.NS_PER_DAY + aux_ref.EDGE_DAY_OFFSET
        assert min(day_of[i] for i in g[f"train_ids_{k}"].tolist()) != start_day
    assert all(len(g[f"test_ids_{k}"]) for k in range(N_EDGE_SPLITS) if k != 6)
    assert 0 < len(g["train_ids_8"]) < len(g["train_ids_0"])


@pytest.mark.parametrize("k", range(N_EDGE_CPK))
def test_card_precision_reproduces_reference_on_edge_frame(golden, k):
    g = golden("split_cpk_edges.npz")
    f, pred = aux_ref.fixture_frame(g)
    nb, cp, mean, sens = aux_ref.card_precision(f["TX_TIME_DAYS"], f["CUSTOMER_ID"], pred, f["TX_FRAUD"],
                                                int(g[f"cpk_topk_{k}"]), bool(g[f"cpk_remove_{k}"]))
    assert not any(sens)            # else the stored result is an accident of pandas' sort
    np.testing.assert_array_equal(np.array(nb), g[f"nb_comp_{k}"])
    np.testing.assert_array_equal(np.array(cp), g[f"cp_{k}"])
    assert mean == float(g[f"mean_{k}"])


def test_edge_frame_reproduces_the_stored_inputs(golden):
    g = golden("split_cpk_edges.npz")
    stored, stored_pred = aux_ref.fixture_frame(g)
    f = aux_ref.edge_frame(int(g["seed"]))
    assert sorted(f) == sorted(stored)
    for name in stored:
        np.testing.assert_array_equal(f[name], stored[name], err_msg=name)
    np.testing.assert_array_equal(aux_ref.edge_predictions(f, int(g["seed"]), tie_safe=True), stored_pred)
    # what the frame is for
    days = np.unique(f["TX_TIME_DAYS"])
    assert days[0] == aux_ref.EDGE_DAY_OFFSET and len(days) == aux_ref.EDGE_DAYS - len(aux_ref.EDGE_REMOVED_DAYS)
    assert not set(days.tolist()) & {aux_ref.EDGE_DAY_OFFSET + d for d in aux_ref.EDGE_REMOVED_DAYS}
    assert len(np.unique(f["CUSTOMER_ID"])) > 3 * 256 and f["CUSTOMER_ID"].min() < 0
    assert 15_000 <= len(f["TX_FRAUD"]) <= 20_000 and 0.02 < f["TX_FRAUD"].mean() < 0.04


def test_tie_unsafe_predictions_are_mostly_tie_sensitive():
    f = aux_ref.edge_frame()
    pred = aux_ref.edge_predictions(f, tie_safe=False)
    for top_k, remove in ((7, True), (100, False)):
        sens = aux_ref.card_precision(f["TX_TIME_DAYS"], f["CUSTOMER_ID"], pred, f["TX_FRAUD"], top_k, remove)[3]
        assert 2 * sum(sens) > len(sens)


def test_card_precision_hand_vector():
    #            day 1: customers 5 (0.5, fraud), 3 (0.5), 9 (0.9)    day 2: 5 (0.1 fraud), 3 (-0.0), 4 (0.0 fraud)
    day = [1, 1, 1, 1, 2, 2, 2, 2]
    cust = [5, 3, 9, 5, 5, 3, 4, 3]
    pred = [0.5, 0.5, 0.9, 0.2, 0.1, -0.0, 0.0, -0.0]
    fraud = [0, 0, 0, 1, 1, 0, 1, 0]
    # top 2 of day 1: 9, then 3 before 5 (tie at 0.5: customer ascending) -> no hit; the tied
    # group {3: 0, 5: 1} straddles the cut with two labels -> tie-sensitive.  top 2 of day 2:
    # 5 (0.1), then 3 (-0.0 == 0.0, customer 3 < 4) -> one hit, tie-sensitive as well
    nb, cp, mean, sens = aux_ref.card_precision(day, cust, pred, fraud, 2, True)
    assert (nb, cp, mean, sens) == ([1, 2], [0.0, 0.5], 0.25, [True, True])
    # top 3 holds every customer of either day: no cut, every compromised customer is a hit
    nb, cp, mean, sens = aux_ref.card_precision(day, cust, pred, fraud, 3, False)
    assert (nb, cp, sens) == ([1, 2], [1 / 3, 2 / 3], [False, False])
    # removal: customer 5 is detected on day 1 (top 3) and its day-2 row is dropped
    nb, cp, _, _ = aux_ref.card_precision(day, cust, pred, fraud, 3, True)
    assert (nb, cp) == ([1, 1], [1 / 3, 1 / 3])
    nb, cp, _, _ = aux_ref.card_precision([1, 2], [5, 5], [0.5, 0.5], [1, 1], 1, True)
    assert (nb, cp) == ([1, 0], [1.0, 0.0])


def test_split_masks_hand_vector():
    D = aux_ref.NS_PER_DAY
    #       row: 0     1      2      3      4      5      6      7      8
    day = [10,   10,   11,    12,    12,    13,    13,    14,    14]
    cust = [1,   2,    3,     4,     3,     4,     5,     5,     6]
    fraud = [1,  0,    0,     1,     0,     0,     1,     0,     0]
    ts = [d * D + 5 for d in day]
    # train = days 10, 11 (d0 = 10): known {1}.  test day 0 = day 13 after delay day 11 (no fraud):
    # rows 5, 6.  test day 1 = day 14 after delay day 12 (customer 4): rows 7, 8 (5's fraud on day
    # 13 is not known yet on day 14)
    train, test = aux_ref.split_masks(ts, day, cust, fraud, 10 * D, 2, 1, 2)
    assert train.tolist() == [True, True, True] + [False] * 6
    assert test.tolist() == [False] * 5 + [True, True, True, True]
    # no delay: test day 0 = day 12 after delay day 11; test day 1 = day 13 knows 4 (day 12)
    train, test = aux_ref.split_masks(ts, day, cust, fraud, 10 * D, 2, 0, 2)
    assert test.tolist() == [False, False, False, True, True, False, True, False, False]
    # ts exactly t_hi is not a train row; an empty train set empties both
    train, _ = aux_ref.split_masks([10 * D, 12 * D], [10, 12], [1, 1], [0, 0], 10 * D, 2, 0, 1)
    assert train.tolist() == [True, False]
    train, test = aux_ref.split_masks(ts, day, cust, fraud, 20 * D, 2, 0, 2)
    assert not train.any() and not test.any()


def test_segment_references_hand_vectors():
    ts = np.array([5, 9, 9, 1, 7, 7, 3], np.int64)
    seg = np.array([0, 3, 3, 4, 7], np.int64)          # segments: [5 9 9] [] [1] [7 7 3]
    assert aux_ref.segment_latest(ts, None, seg).tolist() == [1, -1, 3, 4]
    assert aux_ref.segment_first_in_range(ts, None, seg, 7, 10).tolist() == [1, -1, -1, 4]
    assert aux_ref.segment_first_in_range(ts, None, seg, 1, 6).tolist() == [0, -1, 3, 6]
    assert aux_ref.segment_first_in_range(ts, None, seg, 7, 7).tolist() == [-1, -1, -1, -1]
    perm = np.array([6, 2, 1, 0, 5, 3, 4], np.int32)   # ts[perm] = [3 9 9] [] [5] [7 1 7]
    assert aux_ref.segment_latest(ts, perm, seg).tolist() == [2, -1, 0, 5]
    assert aux_ref.segment_first_in_range(ts, perm, seg, 7, 10).tolist() == [2, -1, -1, 5]
    assert aux_ref.segment_first_in_range(ts, perm, seg, 0, 2).tolist() == [-1, -1, -1, 3]


def test_cdc_decode_hand_vectors():
    raw = [b"\x2f\x12", b"\xff", b"\x00", b"\x80", b"\x00\xff", b"\xff\x7f", b"", b"\x01" * 9,
           b"\x7f" + b"\xff" * 7, b"\x80" + b"\x00" * 7]
    us = [1736940739000000, -1, 0, 999_999, 1_000_000, -1_000_001, -999_999, 1_000_001, 5, 5]
    uns, amt, tsn, bad = aux_ref.cdc_decode(raw, us)
    assert uns.tolist() == [12050, -1, 0, -128, 255, -129, 0, 0, 2 ** 63 - 1, -2 ** 63]
    assert amt[:6].tolist() == [120.5, -0.01, 0.0, -1.28, 2.55, -1.29]
    assert bad.tolist() == [False] * 6 + [True, True, False, False]
    s = 10 ** 9
    assert tsn.tolist() == [1736940739 * s, 0, 0, 0, s, -s, 0, s, 0, 0]
    assert aux_ref.cdc_decode(None, [2_500_000])[:3] == (None, None, np.array([2 * s]))
    uns, amt, tsn, bad = aux_ref.cdc_decode([b"\x01\x00"], None)
    assert (uns.tolist(), amt.tolist(), tsn, bad.tolist()) == ([256], [2.56], None, [False])


def test_dedup_and_compact_hand_vectors():
    key = [7, 8, 7, 7, 9, 8, -3]
    kts = [5, 1, 9, 9, 0, 0, 4]
    #      7: kts 9 twice -> the later (row 3); 8: row 1; 9: row 4; -3: row 6
    assert aux_ref.dedup_latest(key, kts).tolist() == [False, True, False, True, True, False, True]
    assert aux_ref.dedup_latest([], []).tolist() == []
    keep = [1, 0, 1, 1]
    c = aux_ref.cdc_compact(keep, [2 ** 31 - 1, 4, 2 ** 31, -5], [0, 1, 2, 3], [10, 11, 12, 13], [1.5, 2.5, 3.5, 4.5],
                            [0, 1, 7, 0])
    assert c["count"] == 3 and c["row_out"].tolist() == [0, 2, 3]
    assert c["cust"].tolist() == [2 ** 31 - 1, -1, -1] and c["term"].tolist() == [0, 2, 3]
    assert c["ts"].tolist() == [10, 12, 13] and c["amt"].tolist() == [1.5, 3.5, 4.5] and c["fraud"].tolist() == [0, 1, 0]
    c = aux_ref.cdc_compact([0, 0], [1, 2], [1, 2], [1, 2], [1.0, 2.0], None)
    assert c["count"] == 0 and c["row_out"].tolist() == [] and c["fraud"].tolist() == []
