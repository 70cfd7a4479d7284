"""The kernels of csrc/fdx_aux.hip at their edges, against the plain references of
tests/aux_ref.py (pinned to the reference project's own functions by tests/test_aux_ref.py) and
the fixture tests/golden/split_cpk_edges.npz (the reference's get_train_test_set and
card_precision_top_k on aux_ref.edge_frame, written by oracle/gen_split_golden.py).

Everything compares exactly: masks, ids, counts, and cp = hits / top_k as the same double
division.  What the older tests of these kernels (test_gpu_evaluation.py, test_gpu_serving.py)
cannot reach: more customers than one 256-thread block, ties at the top-k cut (the rule is
prediction descending, then customer ascending), top_k beyond the customers present, -0.0
predictions, removed days and day numbering not from 0, empty segments, perm == NULL, more
segments than the capped grid has waves, 64-row chunk boundaries of the ballot search, the bad
paths of decode and dedup, the id narrowing of compact and the nullable arguments of decode.
"""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import aux_ref
from fdx import _lib, evaluation, ops, serving

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
N_SPLITS = 9
N_CPK = 12


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


@functools.lru_cache(maxsize=None)
def _edge():
    """(columns, DataFrame) of the edge frame, built once"""
    f = aux_ref.edge_frame()
    df = pd.DataFrame(f)
    df["TX_DATETIME"] = df["TX_DATETIME"].astype("datetime64[ns]")
    return f, df


def _pred_frame(day, cust, pred, fraud):
    return pd.DataFrame({"TX_TIME_DAYS": np.asarray(day, np.int64), "CUSTOMER_ID": np.asarray(cust, np.int64),
                         "TX_FRAUD": np.asarray(fraud, np.int64), "predictions": np.asarray(pred, np.float64)})


def _check_cp(day, cust, pred, fraud, top_k, remove):
    """evaluation.card_precision_top_k == aux_ref.card_precision; -> the reference's result"""
    nb, cp, mean = evaluation.card_precision_top_k(_pred_frame(day, cust, pred, fraud), top_k, remove)
    rnb, rcp, rmean, sens = aux_ref.card_precision(day, cust, pred, fraud, top_k, remove)
    assert nb == rnb, f"top_k {top_k} remove {remove}"
    assert cp == rcp, f"top_k {top_k} remove {remove}"
    assert mean == rmean
    return rnb, rcp, sens


# ------------------------------------------------------------------ split
def _split_direct(dev, ts, day, cust, fraud, t_lo, delta_train, delta_delay, delta_test):
    """fdx_train_test_split on the raw columns (customer ids made dense on the host)"""
    n = len(ts)
    ids, dense = np.unique(np.asarray(cust, np.int64), return_inverse=True)
    n_cust = len(ids)
    ts_d, day_d = T(np.asarray(ts, np.int64), torch.int64, dev), T(np.asarray(day, np.int32), torch.int32, dev)
    cust_d = T(dense.astype(np.int32), torch.int32, dev)
    fraud_d = T((np.asarray(fraud) != 0).astype(np.uint8), torch.uint8, dev)
    train = torch.zeros(n, dtype=torch.uint8, device=dev)
    test = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = ops.workspace(n_cust * 5 + 64, dev)
    dmin = ctypes.c_int32(0)
    _lib.check(_lib.load().fdx_train_test_split(
        ops._ptr(ts_d), ops._ptr(day_d), ops._ptr(cust_d), ops._ptr(fraud_d), n, n_cust, int(t_lo),
        int(t_lo) + int(delta_train) * aux_ref.NS_PER_DAY, int(delta_train), int(delta_delay), int(delta_test),
        ops._ptr(train), ops._ptr(test), ops._ptr(ws), ws.numel(), ctypes.byref(dmin), ops._s()), "fdx_train_test_split")
    return train.cpu().numpy().astype(bool), test.cpu().numpy().astype(bool)


@pytest.mark.parametrize("k", range(N_SPLITS))
def test_split_on_edge_frame_matches_reference(dev, golden, k):
    g = golden("split_cpk_edges.npz")
    _, df = _edge()
    dtr, dde, dte = (int(d) for d in g[f"split_deltas_{k}"])
    ratio, random_state = g[f"split_sampling_{k}"]
    tr, te = evaluation.get_train_test_set(df, pd.Timestamp(int(g[f"split_start_ns_{k}"])), dtr, dde, dte,
                                           sampling_ratio=float(ratio), random_state=int(random_state))
    np.testing.assert_array_equal(tr.TRANSACTION_ID.values, g[f"train_ids_{k}"])
    np.testing.assert_array_equal(te.TRANSACTION_ID.values, g[f"test_ids_{k}"])


@pytest.mark.parametrize("k", range(N_SPLITS - 1))  # the last case is case 0 subsampled on the host
def test_split_kernel_matches_plain_reference(dev, golden, k):
    g = golden("split_cpk_edges.npz")
    f, _ = _edge()
    cols = (f["TX_DATETIME"], f["TX_TIME_DAYS"], f["CUSTOMER_ID"], f["TX_FRAUD"])
    args = (int(g[f"split_start_ns_{k}"]), *(int(d) for d in g[f"split_deltas_{k}"]))
    train, test = _split_direct(dev, *cols, *args)
    rtrain, rtest = aux_ref.split_masks(*cols, *args)
    np.testing.assert_array_equal(train, rtrain)
    np.testing.assert_array_equal(test, rtest)


def test_split_of_an_empty_frame(dev):
    e = np.zeros(0, np.int64)
    train, test = _split_direct(dev, e, e, e, e, 0, 7, 7, 7)
    rtrain, rtest = aux_ref.split_masks(e, e, e, e, 0, 7, 7, 7)
    assert train.shape == rtrain.shape == (0,) and test.shape == rtest.shape == (0,)


def test_split_customer_with_frauds_in_training_and_in_the_delay_period(dev):
    """A customer known from the train rows stays out of every test day, also when it has a
    later fraud on a delay day (the later day must not replace the earlier knowledge); a
    customer with frauds on two delay days is out from the first of them on."""
    rng = np.random.default_rng(3)
    D = aux_ref.NS_PER_DAY
    n, n_cust = 3000, 700
    day = np.sort(rng.integers(40, 64, n))
    ts = day * D + rng.integers(0, 86_400, n) * 10 ** 9
    cust = rng.integers(0, n_cust, n) * 3 - 50
    fraud = (rng.random(n) < 0.01).astype(np.int64)
    # train days 42..45, delay days 45 + [0, 6), test days 49 + [0, 6)
    extra_day = np.array([43, 47, 49, 50, 52,   46, 50, 49, 50, 51, 52])
    extra_cust = np.array([7] * 5 + [10] * 6)
    extra_fraud = np.array([1, 1, 0, 0, 0,      1, 1, 0, 0, 0, 0])
    day = np.concatenate([day, extra_day])
    ts = np.concatenate([ts, extra_day * D + 12 * 3600 * 10 ** 9])
    cust = np.concatenate([cust, extra_cust])
    fraud = np.concatenate([fraud, extra_fraud])
    o = np.argsort(ts, kind="stable")
    ts, day, cust, fraud = ts[o], day[o], cust[o], fraud[o]
    args = (42 * D, 4, 3, 6)
    train, test = _split_direct(dev, ts, day, cust, fraud, *args)
    rtrain, rtest = aux_ref.split_masks(ts, day, cust, fraud, *args)
    assert rtest.any() and rtrain.any()
    assert not rtest[cust == 7].any()
    # customer 10: frauds on delay days 46 and 50, known from test day 50 = 49 + 1 on: its day-49 row is a test row
    assert rtest[(cust == 10) & (day == 49)].all() and not rtest[(cust == 10) & (day > 49)].any()
    np.testing.assert_array_equal(train, rtrain)
    np.testing.assert_array_equal(test, rtest)


# ------------------------------------------------------------------ Card-Precision@k
@pytest.mark.parametrize("k", range(N_CPK))
def test_card_precision_on_edge_frame_matches_reference(dev, golden, k):
    g = golden("split_cpk_edges.npz")
    f, pred = aux_ref.fixture_frame(g)
    pdf = _pred_frame(f["TX_TIME_DAYS"], f["CUSTOMER_ID"], pred, f["TX_FRAUD"])
    nb, cp, mean = evaluation.card_precision_top_k(pdf, int(g[f"cpk_topk_{k}"]), bool(g[f"cpk_remove_{k}"]))
    np.testing.assert_array_equal(np.array(nb), g[f"nb_comp_{k}"])
    np.testing.assert_array_equal(np.array(cp), g[f"cp_{k}"])
    assert mean == float(g[f"mean_{k}"])


@pytest.mark.parametrize("remove", [True, False])
def test_card_precision_ties_at_the_cut_go_by_customer_ascending(dev, remove):
    """Tie-sensitive inputs: the group at the cut mixes labels on most days, so the result
    depends on the order among equal predictions -- the documented one, customer ascending."""
    f, _ = _edge()
    pred = aux_ref.edge_predictions(f, tie_safe=False)
    n_sensitive = 0
    for top_k in (1, 7, 100, 256, 257, 2000):
        _, _, sens = _check_cp(f["TX_TIME_DAYS"], f["CUSTOMER_ID"], pred, f["TX_FRAUD"], top_k, remove)
        n_sensitive += sum(sens)
    assert n_sensitive > 100   # of 6 * 47 days


def _negative_zero_case():
    """300 customers on two days.  Customers 10, 11, 12 (compromised) have only -0.0
    predictions, 0..9 have 0.0, customer 20 has a -0.0 row beside a 0.3 row, the rest are
    positive; the five largest predictions belong to genuine customers."""
    n_cust = 300
    cust = np.arange(n_cust)
    pred = 0.1 + 0.8 * (cust * 37 % n_cust) / n_cust     # distinct, in [0.1, 0.9)
    pred[:10] = 0.0
    pred[10:13] = -0.0
    fraud = np.zeros(n_cust, np.int64)
    fraud[10:13] = 1
    fraud[[50, 60, 70]] = 1
    top5 = np.argsort(-pred)[:5]
    assert not fraud[top5].any()
    day = np.concatenate([np.full(n_cust, 3), np.full(n_cust, 4), [3, 4]])
    cust = np.concatenate([cust, cust, [20, 20]])
    pred = np.concatenate([pred, pred, [-0.0, -0.0]])
    fraud = np.concatenate([fraud, fraud, [0, 0]])
    return day, cust, pred, fraud


@pytest.mark.parametrize("top_k, remove", [(5, False), (5, True), (295, False), (295, True)])
def test_card_precision_negative_zero_ranks_as_zero(dev, top_k, remove):
    """-0.0 passes the wrapper's `min() < 0` check; its bit pattern 0x8000... is above every
    positive double's, so a kernel comparing raw patterns would rank it first."""
    day, cust, pred, fraud = _negative_zero_case()
    assert np.signbit(pred).sum() == 8 and pred.min() == 0.0
    _, cp, _ = _check_cp(day, cust, pred, fraud, top_k, remove)
    if top_k == 5:
        assert cp == [0.0, 0.0]           # ranked first, the three -0.0 customers would make it 0.6
    elif not remove:
        assert cp == [3 / 295, 3 / 295]   # 287 positive customers, then zeros 0..7: 10, 11, 12 stay out


def test_card_precision_top_k_at_and_beyond_the_customers_present(dev):
    f, _ = _edge()
    sel = f["TX_TIME_DAYS"] < aux_ref.EDGE_DAY_OFFSET + 4
    day, cust, fraud = f["TX_TIME_DAYS"][sel], f["CUSTOMER_ID"][sel], f["TX_FRAUD"][sel]
    pred = aux_ref.edge_predictions(f, tie_safe=False)[sel]
    present = [len(set(cust[day == d].tolist())) for d in np.unique(day)]
    for top_k in (min(present) - 1, min(present), max(present), max(present) + 1, 100_000):
        for remove in (True, False):
            nb, cp, _ = _check_cp(day, cust, pred, fraud, top_k, remove)
            if top_k >= max(present) and not remove:
                assert cp == [b / top_k for b in nb]     # every compromised customer is a hit


def test_card_precision_day_with_every_customer_detected_and_single_customer(dev):
    #      day 1: 4 and 8 compromised, both in the top 3 -> detected; day 2 holds only them
    day = [1, 1, 1, 1, 2, 2, 2, 3, 3]
    cust = [4, 8, 6, 4, 8, 4, 4, 6, 8]
    pred = [0.9, 0.8, 0.1, 0.2, 0.7, 0.6, 0.5, 0.3, 0.4]
    fraud = [1, 1, 0, 0, 1, 1, 0, 1, 1]
    nb, cp, _ = _check_cp(day, cust, pred, fraud, 3, True)
    assert (nb, cp) == ([2, 0, 1], [2 / 3, 0.0, 1 / 3])
    nb, cp, _ = _check_cp(day, cust, pred, fraud, 3, False)
    assert (nb, cp) == ([2, 2, 2], [2 / 3, 2 / 3, 2 / 3])
    for top_k in (1, 2):
        for remove in (True, False):
            for label in (0, 1):
                nb, cp, _ = _check_cp([9], [-77], [0.25], [label], top_k, remove)
                assert (nb, cp) == ([label], [label / top_k])


@pytest.mark.parametrize("bad", [-1e-300, -0.5, float("nan")])
def test_card_precision_refuses_negative_and_nan_predictions(dev, bad):
    pdf = _pred_frame([1, 1, 2], [1, 2, 3], [0.5, bad, 0.25], [0, 1, 0])
    with pytest.raises(_lib.FdxUnsupported):
        evaluation.card_precision_top_k(pdf, 2)


# ------------------------------------------------------------------ segment selections
@functools.lru_cache(maxsize=None)
def _segments():
    """-> (seg_off, ts by position).  Hand-made segments first, then the lengths around the
    64-lane chunk (mixed), then 20,000 segments of 0..3 rows: more segments than the capped
    grid's 16,384 waves.  Timestamps are small integers (heavy ties)."""
    rng = np.random.default_rng(17)
    hand = []
    a = np.ones(200, np.int64)
    a[[70, 140]] = 9                      # the maximum tied in two different chunks, none in the first
    hand.append(a)
    a = np.ones(200, np.int64)
    a[[63, 64, 199]] = 9                  # ... on both sides of a chunk boundary
    hand.append(a)
    a = np.full(100, 4, np.int64)
    a[99] = 2                             # the only row in [2, 4): the last one of a partial chunk
    hand.append(a)
    a = np.full(130, 4, np.int64)
    a[64:] = 3                            # the rows in [2, 4) start exactly at position 64
    hand.append(a)
    a = np.full(128, 4, np.int64)
    a[127] = 3                            # ... the last lane of the last full chunk
    hand.append(a)
    hand.append(np.full(3, I64_MIN, np.int64))                        # latest of all-INT64_MIN rows
    hand.append(np.array([I64_MIN, I64_MAX - 1, I64_MAX - 1, 0, I64_MIN], np.int64))
    hand.append(np.array([4, I64_MAX - 1, I64_MIN], np.int64))
    lens = np.concatenate([[0, 1, 63, 64, 65, 127, 128, 129, 1000, 0, 0, 1037],
                           rng.permutation(np.repeat([0, 1, 63, 64, 65, 127, 128, 129], 3)),
                           rng.integers(0, 4, 20_000), [0, 65, 0]])
    parts = hand + [rng.integers(0, 7, int(m)) for m in lens]
    seg_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return seg_off, np.concatenate(parts).astype(np.int64)


RANGES = [(2, 4), (3, 3), (7, 100), (10, 100), (0, 1), (I64_MIN, I64_MIN + 1), (I64_MAX - 1, I64_MAX), (I64_MIN, I64_MAX),
          (6, 7)]


@functools.lru_cache(maxsize=None)
def _segment_case(with_perm):
    seg_off, tsp = _segments()
    n = len(tsp)
    if not with_perm:
        return seg_off, tsp, None
    perm = np.random.default_rng(23).permutation(n).astype(np.int32)
    ts = np.empty(n, np.int64)
    ts[perm] = tsp
    return seg_off, ts, perm


@pytest.mark.parametrize("with_perm", [True, False], ids=["perm", "noperm"])
def test_segment_latest_edges(dev, with_perm):
    seg_off, ts, perm = _segment_case(with_perm)
    assert len(seg_off) - 1 > 16_384 and (np.diff(seg_off) == 0).sum() > 1000
    ref = aux_ref.segment_latest(ts, perm, seg_off)
    got = serving.segment_latest(T(ts, torch.int64, dev), None if perm is None else T(perm, torch.int32, dev),
                                 T(seg_off, torch.int64, dev)).cpu().numpy()
    if perm is None:
        assert ref[:2].tolist() == [70, 200 + 63] and ref[5] == seg_off[5]
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("with_perm", [True, False], ids=["perm", "noperm"])
def test_segment_first_in_range_edges(dev, with_perm):
    seg_off, ts, perm = _segment_case(with_perm)
    ts_d, seg_d = T(ts, torch.int64, dev), T(seg_off, torch.int64, dev)
    perm_d = None if perm is None else T(perm, torch.int32, dev)
    for lo, hi in RANGES:
        ref = aux_ref.segment_first_in_range(ts, perm, seg_off, lo, hi)
        got = serving.segment_first_in_range(ts_d, perm_d, seg_d, lo, hi).cpu().numpy()
        if perm is None and (lo, hi) == (2, 4):
            assert ref[2:5].tolist() == [seg_off[2] + 99, seg_off[3] + 64, seg_off[4] + 127]
        if lo == hi or (lo, hi) == (10, 100):
            assert (ref == -1).all()              # a range holding nothing
        if (lo, hi) == (7, 100):
            assert (ref >= 0).sum() == 2          # only the hand-made 9s
        np.testing.assert_array_equal(got, ref, err_msg=f"[{lo}, {hi})")


def test_segment_selections_without_segments(dev):
    ts = T(np.arange(4), torch.int64, dev)
    seg = T(np.zeros(1), torch.int64, dev)
    assert serving.segment_latest(ts, None, seg).numel() == 0
    assert serving.segment_first_in_range(ts, None, seg, 0, 9).numel() == 0


# ------------------------------------------------------------------ CDC decode
def _encodings():
    """(bytes, value) pairs: the smallest and largest value of every length 1..8, 0, -1 as 0xFF,
    sign-padded (non-minimal) encodings, and random values of random lengths (several blocks)."""
    rng = np.random.default_rng(29)
    vals = []
    for ln in range(1, 9):
        lo, hi = -(1 << (8 * ln - 1)), (1 << (8 * ln - 1)) - 1
        vals += [(v, ln) for v in (lo, hi, lo + 1, hi - 1, 0, -1, 1)]
    vals += [(5, 3), (-5, 3), (1, 8), (-1, 8), (-128, 8), (127, 2), (-129, 8), (12050, 2), (12050, 5),
             (2 ** 53 - 1, 7), (-(2 ** 53) + 1, 7), (2 ** 53 - 1, 8), (-(2 ** 53) + 1, 8), (10 ** 10 - 1, 5), (-(10 ** 10) + 1, 5)]
    for _ in range(700):
        ln = int(rng.integers(1, 9))
        bits = min(8 * ln - 1, 53)
        vals.append((int(rng.integers(-(1 << bits) + 1, 1 << bits)), ln))
    return [v.to_bytes(ln, "big", signed=True) for v, ln in vals], [v for v, _ in vals]


def _us_values(n):
    special = [-1, 0, 1, 999_999, 1_000_000, 1_000_001, -999_999, -1_000_000, -1_000_001, 1_999_999, 2_000_000,
               1736940739000000, 1736940739999999, -1736940739999999, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2,
               9_223_372_036_000_000, 9_223_372_035_999_999, -9_223_372_036_000_000, -9_223_372_035_999_999]
    rng = np.random.default_rng(31)
    rand = rng.integers(-1_760_000_000_000_000, 1_760_000_000_000_000, n - len(special))
    return np.concatenate([np.array(special, np.int64), rand])


def _blob(raw, dev):
    lens = np.array([len(b) for b in raw], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    blob = np.frombuffer(b"".join(raw) or b"\0", np.uint8).copy()
    return T(blob, torch.uint8, dev), T(off, torch.int64, dev)


def _check_decode(raw, values, us, got):
    uns, amt, tsn = got
    runs, ramt, rtsn, rbad = aux_ref.cdc_decode(raw, us)
    if raw is None:
        assert uns is None and amt is None
    else:
        assert not rbad.any() and runs.tolist() == values
        np.testing.assert_array_equal(uns.cpu().numpy(), runs)
        small = np.abs(runs.astype(np.float64)) < 2.0 ** 53   # Decimal / 100 == double / 100.0 by construction
        assert small.sum() > 700
        np.testing.assert_array_equal(amt.cpu().numpy()[small], ramt[small])
        # beyond 2^53 the documented amount is the double division of the rounded value
        np.testing.assert_array_equal(amt.cpu().numpy(), runs.astype(np.float64) / 100.0)
    if us is None:
        assert tsn is None
    else:
        np.testing.assert_array_equal(tsn.cpu().numpy(), rtsn)


def test_cdc_decode_every_length_sign_and_padding(dev):
    raw, values = _encodings()
    us = _us_values(len(raw))
    assert {len(b) for b in raw} == set(range(1, 9)) and len(raw) > 3 * 256
    b, off = _blob(raw, dev)
    us_d = T(us, torch.int64, dev)
    _check_decode(raw, values, us, serving.cdc_decode(b, off, us_d))
    _check_decode(raw, values, None, serving.cdc_decode(b, off, None))      # amount only
    _check_decode(None, None, us, serving.cdc_decode(None, None, us_d))    # timestamp only


@pytest.mark.parametrize("field", [b"", b"\x00" * 9, b"\xff" * 12])
def test_cdc_decode_refuses_fields_of_0_or_more_than_8_bytes(dev, field):
    raw = [b"\x01", b"\x02\x03", field, b"\x7f"]
    b, off = _blob(raw, dev)
    assert aux_ref.cdc_decode(raw, None)[3].tolist() == [False, False, True, False]
    with pytest.raises(_lib.FdxUnsupported):
        serving.cdc_decode(b, off, None)
    with pytest.raises(_lib.FdxUnsupported):
        serving.cdc_decode(b, off, T(np.arange(4), torch.int64, dev))


# ------------------------------------------------------------------ dedup
def _check_dedup(dev, key, kts):
    key, kts = np.asarray(key, np.int64), np.asarray(kts, np.int64)
    got = serving.dedup_latest(T(key, torch.int64, dev), T(kts, torch.int64, dev)).cpu().numpy().astype(bool)
    np.testing.assert_array_equal(got, aux_ref.dedup_latest(key, kts))
    return got


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 4097])
def test_dedup_at_the_table_capacity_edges(dev, n):
    """the table holds the next power of two >= 2 n slots: n at and past a power of two"""
    rng = np.random.default_rng(n)
    key = rng.integers(-(n // 3) - 2, n // 3 + 2, n) * 1_000_003
    key[key == -1] = -2
    keep = _check_dedup(dev, key, rng.integers(0, 5, n))
    assert keep.sum() == len(np.unique(key))
    keep = _check_dedup(dev, (np.arange(n) - n // 2) * 2, rng.integers(0, 3, n))   # all keys distinct (even: none is -1)
    assert keep.all()


def test_dedup_one_key_many_records(dev):
    rng = np.random.default_rng(41)
    kts = rng.integers(0, 50, 5000)              # tied in groups of ~100
    keep = _check_dedup(dev, np.full(5000, 123_456_789), kts)
    assert keep.sum() == 1 and keep[np.nonzero(kts == kts.max())[0][-1]]
    keep = _check_dedup(dev, np.full(5000, I64_MIN), np.zeros(5000, np.int64))   # all tied: the last record
    assert keep.nonzero()[0].tolist() == [4999]


def test_dedup_extreme_keys_and_timestamps(dev):
    rng = np.random.default_rng(43)
    n = 3000
    key = rng.choice(np.array([I64_MIN, I64_MIN + 1, -2, 0, 1, I64_MAX - 1, I64_MAX, -(2 ** 40), 2 ** 40], np.int64), n)
    kts = rng.choice(np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64), n)
    keep = _check_dedup(dev, key, kts)
    assert keep.sum() == 9
    _check_dedup(dev, key, np.full(n, I64_MIN))
    _check_dedup(dev, key, np.full(n, I64_MAX))


@pytest.mark.parametrize("n, at", [(1, 0), (300, 0), (300, 299), (4097, 4096)])
def test_dedup_refuses_key_minus_one(dev, n, at):
    key = np.arange(n, dtype=np.int64) % 7
    key[at] = -1
    with pytest.raises(_lib.FdxUnsupported):
        serving.dedup_latest(T(key, torch.int64, dev), T(np.zeros(n, np.int64), torch.int64, dev))


# ------------------------------------------------------------------ compact
def _compact(dev, keep, cust, term, ts, amt, fraud):
    """fdx_cdc_compact as StreamScorer.score_cdc calls it -> the kept columns, cut to the count"""
    n = len(keep)
    L = _lib.load()
    i32 = lambda: torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)  # noqa: E731
    out = dict(cust=i32(), term=i32(), ts=torch.zeros(max(n, 1), dtype=torch.int64, device=dev),
               amt=torch.zeros(max(n, 1), dtype=torch.float64, device=dev),
               fraud=torch.full((max(n, 1),), 9, dtype=torch.uint8, device=dev), row_out=i32())
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws = ops.workspace(L.fdx_cdc_compact_workspace_size(n), dev)
    P = ops._ptr
    # the inputs stay referenced until the call has run (a temporary's block could be handed out again)
    keep_d = T(np.asarray(keep, np.uint8), torch.uint8, dev)
    cust_d, term_d = T(np.asarray(cust, np.int64), torch.int64, dev), T(np.asarray(term, np.int64), torch.int64, dev)
    ts_d, amt_d = T(np.asarray(ts, np.int64), torch.int64, dev), T(np.asarray(amt, np.float64), torch.float64, dev)
    fraud_d = None if fraud is None else T(np.asarray(fraud, np.uint8), torch.uint8, dev)
    _lib.check(L.fdx_cdc_compact(P(keep_d), n, P(cust_d), P(term_d), P(ts_d), P(amt_d), P(fraud_d), P(out["cust"]),
                                 P(out["term"]), P(out["ts"]), P(out["amt"]), P(out["fraud"]), P(out["row_out"]),
                                 P(count), P(ws), ws.numel(), ops._s()), "fdx_cdc_compact")
    m = int(count.item())
    assert 0 <= m <= n
    res = {k: v[:m].cpu().numpy() for k, v in out.items()}
    res["count"] = m
    return res


def _check_compact(dev, keep, with_fraud=True, seed=0):
    rng = np.random.default_rng(seed)
    n = len(keep)
    ids = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, -5, 2 ** 31 - 2, 2 ** 32 + 3, -1, I64_MIN, I64_MAX, 12345], np.int64)
    cust, term = rng.choice(ids, n), rng.choice(ids, n)
    ts = rng.integers(I64_MIN, I64_MAX, n)
    amt = rng.normal(0, 1e6, n)
    fraud = rng.integers(0, 3, n).astype(np.uint8) if with_fraud else None   # any non-zero byte is a fraud
    got = _compact(dev, keep, cust, term, ts, amt, fraud)
    ref = aux_ref.cdc_compact(keep, cust, term, ts, amt, fraud)
    assert got["count"] == ref["count"]
    for k in ("row_out", "cust", "term", "ts", "amt", "fraud"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# the scan behind the compaction works in blocks of 256 threads x 16 items = 4,096 rows; 1,500 and
# 3,100 are the segment lengths test_gpu_scan.py uses
COMPACT_SIZES = [1, 2, 255, 256, 257, 1500, 3100, 4095, 4096, 4097, 8191, 8192, 8193, 12_289]


@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_cdc_compact_across_the_scan_block_edges(dev, n):
    rng = np.random.default_rng(n)
    one_first, one_last, one_mid = (np.zeros(n, np.uint8) for _ in range(3))
    one_first[0], one_last[n - 1], one_mid[n // 2] = 1, 1, 3            # any non-zero byte keeps
    for j, keep in enumerate([np.ones(n, np.uint8), np.zeros(n, np.uint8), one_first, one_last, one_mid,
                              (rng.random(n) < 0.5).astype(np.uint8), (rng.random(n) < 0.02).astype(np.uint8)]):
        _check_compact(dev, keep, with_fraud=j % 2 == 0, seed=n + j)


def test_cdc_compact_narrows_ids_outside_int32(dev):
    keep = [1, 1, 0, 1, 1]
    got = _compact(dev, keep, [2 ** 31 - 1, 2 ** 31, 7, -5, 0], [-5, 2 ** 31 - 1, 7, 2 ** 31, 3], [1, 2, 3, 4, 5],
                   [1.0, 2.0, 3.0, 4.0, 5.0], None)
    assert got["count"] == 4 and got["row_out"].tolist() == [0, 1, 3, 4]
    assert got["cust"].tolist() == [2 ** 31 - 1, -1, -1, 0] and got["term"].tolist() == [-1, 2 ** 31 - 1, -1, 3]
    assert got["fraud"].tolist() == [0, 0, 0, 0] and got["ts"].tolist() == [1, 2, 4, 5]


def test_cdc_compact_of_an_empty_batch(dev):
    e = np.zeros(0, np.int64)
    assert _compact(dev, np.zeros(0, np.uint8), e, e, e, np.zeros(0), None)["count"] == 0
