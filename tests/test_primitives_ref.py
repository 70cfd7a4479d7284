"""The builders and references of primitives_ref.py, checked on the CPU: every input reaches the
regime it is named for (the pattern of test_gpu_flag_edges.test_inputs_reach_both_regimes), the
digit-plan model matches the schedule csrc/fdx_rekey.hip documents, and the key widths the GPU
tests run cover every plan.  Reference calls: feature_transformation.ipynb:1092-1093, :2435-2436
(the regrouping the re-key replaces)."""
import numpy as np
import pytest

import oracle
import primitives_ref as R


def test_digit_plan_table():
    """The schedule as the issue and csrc/fdx_rekey.hip state it, width by width."""
    want = {}
    for bits, plan in ((range(1, 9), (1, 0)), ([9], (1, 1)), (range(10, 17), (2, 0)), ([17], (2, 1)), ([18], (2, 2)),
                       (range(19, 25), (3, 0)), ([25], (3, 1)), ([26], (3, 2)), ([27], (3, 3)), (range(28, 32), (4, 0))):
        for b in bits:
            want[b] = plan
    assert sorted(want) == list(range(1, 32))
    for b in range(1, 32):
        assert R.digit_plan(b) == want[b], b
        sh = R.digit_shifts(b)  # the passes tile the key's bits from 0 up, without a hole
        assert sh[0][0] == 0 and all(sh[i][0] + sh[i][1] == sh[i + 1][0] for i in range(len(sh) - 1))
        assert sh[-1][0] + sh[-1][1] >= b
    assert R.digit_plan(64) == (8, 0)  # the 64-bit argsort


def test_key_widths_cover_every_plan():
    """Listed, so that a change of the plan (or of the widths a test runs) fails here."""
    reachable = {R.digit_plan(b) for b in range(1, 32)}
    assert reachable == R.PLANS_1_TO_31 and len(reachable) == 10
    assert {b: R.digit_plan(b) for b in R.PARITY_KEY_BITS} == {1: (1, 0), 8: (1, 0), 9: (1, 1), 16: (2, 0), 17: (2, 1),
                                                              18: (2, 2), 21: (3, 0), 25: (3, 1)}
    assert {b: R.digit_plan(b) for b in R.NEW_KEY_BITS} == {10: (2, 0), 19: (3, 0), 24: (3, 0), 26: (3, 2), 27: (3, 3),
                                                           28: (4, 0), 31: (4, 0)}
    assert {R.digit_plan(b) for b in R.PARITY_KEY_BITS + R.NEW_KEY_BITS} == R.PLANS_1_TO_31
    # what the earlier suite never took: two or three 9-bit passes before an 8-bit one, a fourth pass
    assert R.digit_shifts(26) == [(0, 9), (9, 9), (18, 8)] and R.digit_shifts(27) == [(0, 9), (9, 9), (18, 9)]
    assert R.digit_shifts(28) == [(0, 8), (8, 8), (16, 8), (24, 8)]


def test_scan_sizes_and_inputs():
    P = [-(-m // R.TILE) for m in R.SCAN_SIZES]
    assert 256 in P and 257 in P and max(P) == 514  # one trip of the carry loop, its second, its third
    rng = np.random.default_rng(0)
    m = R.SCAN_SIZES[-1]
    x = R.scan_input("u32", m, rng)
    assert int(x.astype(np.uint64).sum()) > 1 << 32  # the true total wraps
    assert int(R.scan_input("u16", m, rng).astype(np.uint64).sum()) > 1 << 32
    assert int(R.scan_input("one", m, rng).sum()) == m and not R.scan_input("zero", m, rng).any()
    ref = R.scan_ref(x)
    assert ref[0] == 0 and ref.dtype == np.uint32
    tot = 0
    for i in range(0, 5000):  # the model against plain Python integers
        assert int(ref[i]) == tot % (1 << 32)
        tot += int(x[i])
    big = np.full(3, 0xFFFFFFFF, np.uint32)
    np.testing.assert_array_equal(R.scan_ref(big), np.array([0, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32))


@pytest.mark.parametrize("p", range(8))
def test_byte_keys_differ_in_one_byte_only(p):
    k = R.argsort_keys(f"byte{p}", 17 * 4096 + 17, np.random.default_rng(p)).view(np.uint64)
    mask = np.uint64(0xFF) << np.uint64(8 * p)
    assert not (k & ~mask).any()
    assert len(np.unique(k)) == 256  # every digit of the decisive pass, many ties each
    if p == 7:
        assert (k.view(np.int64) < 0).any() and (k.view(np.int64) >= 0).any()  # the sign is in it


def test_argsort_classes():
    rng = np.random.default_rng(1)
    n = 4097
    full = R.argsort_keys("full", n, rng)
    assert set([R.I64_MIN, R.I64_MAX, -1, 0, 1]) <= set(full.tolist())
    assert len(np.unique(R.argsort_keys("equal", n, rng))) == 1
    assert len(np.unique(R.argsort_keys("two", n, rng))) == 2
    assert (np.diff(R.argsort_keys("sorted", n, rng)) >= 0).all()
    assert (np.diff(R.argsort_keys("descending", n, rng)) < 0).all()
    lo = R.argsort_keys("low32_equal", n, rng)
    assert len(np.unique(lo & 0xFFFFFFFF)) == 1 and len(np.unique(lo >> 32)) > n // 2 and (lo < 0).any()
    hi = R.argsort_keys("high32_equal", n, rng)
    assert len(np.unique(hi >> 32)) == 1 and len(np.unique(hi & 0xFFFFFFFF)) > n // 2
    for kind in R.ARGSORT_KINDS:
        for m in (1, 2, 5):
            assert R.argsort_keys(kind, m, rng).shape == (m,)


def test_dense_classes():
    rng = np.random.default_rng(2)
    for n in R.N_EDGE:
        assert len(np.unique(R.dense_keys("equal", n, rng))) == 1
        assert len(np.unique(R.dense_keys("distinct", n, rng))) == n
        k = R.dense_keys("tile_edge", n, rng)
        s = np.sort(k)
        first = np.flatnonzero(np.r_[False, s[1:] != s[:-1]])
        assert first.tolist() == [p for p in R.DENSE_EDGE_POS if p < n]
    ext = R.dense_keys("extremes", 4097, rng)
    assert set(ext.tolist()) == {R.I64_MIN, R.I64_MAX, 0, 1, -1}
    assert not (np.sort(R.dense_keys("tile_edge", 4097, rng)) == R.dense_keys("tile_edge", 4097, rng)).all()


def test_rekey_keys_reach_both_ends():
    rng = np.random.default_rng(3)
    for bits in R.NEW_KEY_BITS:
        k = R.rekey_keys(bits, 3 * 4096 + 17, rng)
        assert k.dtype == np.int32 and k.min() == 0 and k.max() == (1 << bits) - 1
        for shift, db in R.digit_shifts(bits):  # every pass sees more than one digit
            assert len(np.unique((k.astype(np.int64) >> shift) & ((1 << db) - 1))) > 1
        assert R.rekey_keys(bits, 1, rng).tolist() == [(1 << bits) - 1]
    neg = R.with_negative_ids(R.rekey_keys(31, 3 * 4096 + 17, rng), rng)
    assert 0 < np.count_nonzero(neg < 0) < len(neg)


def test_seg_patterns():
    rng = np.random.default_rng(4)
    assert {n % 4 for n in R.SEG_SIZES} == {0, 1, 2, 3} and {n % 4 for n in R.SEG_SIZES if n >= 4} >= {0, 1, 3}
    for n in R.SEG_SIZES:
        for name in R.SEG_PATTERNS:
            k, nk = R.seg_pattern(name, n, rng)
            assert k.dtype == np.int32 and len(k) == n and (np.diff(k) >= 0).all() and 0 <= k[0] and k[-1] < nk
            off = R.seg_off_ref(k, nk)
            assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
            np.testing.assert_array_equal(np.diff(off), np.bincount(k, minlength=nk))
            absent = np.diff(off) == 0
            if name == "first_gt0":
                assert k[0] > 0
            elif name == "last_lt":
                assert k[-1] < nk - 1
            elif name == "gap":  # a run of at least SEG_GAP absent keys
                run = np.diff(np.flatnonzero(np.r_[True, ~absent, True])) - 1
                assert run.max() >= R.SEG_GAP
                if n > 1:
                    assert (np.diff(k) > R.SEG_GAP).any()  # between two rows
            elif name == "single":
                assert len(np.unique(k)) == 1 and 0 < k[0] < nk - 1
            elif name == "one_key":
                assert nk == 1
            else:
                assert nk == n and not absent.any()
            t = R.with_out_of_range_tail(k, nk)
            assert len(t) == n + 8 and np.count_nonzero((t < 0) | (t >= nk)) == 8 and (t < 0).any() and (t >= nk).any()


def test_keyseg_and_range_inputs():
    rng = np.random.default_rng(5)
    for nk in R.KEYSEG_N_KEYS:
        k = R.keyseg_keys(nk, R.KEYSEG_N, rng)
        assert k.min() == 0 and k.max() == nk - 1
        b = R.keyseg_keys(nk, R.KEYSEG_N, rng, bad=True)
        assert {R.I32_MIN, -1, R.I32_MAX} <= set(b.tolist()) and (b == nk).any()
        assert R.oor_count(b, 0, nk) == 40 and b[0] == nk - 1 and b[-1] == 0
    assert -(-((1 << 20) + 2) // R.TILE) > 256  # the histogram's scan takes the carry loop's second trip
    for n in R.OOR_SIZES:
        for lo, hi in R.OOR_RANGES:
            for lay in R.OOR_LAYOUTS:
                k, pos = R.oor_keys(n, lo, hi, lay, rng)
                assert k.dtype == np.int32 and len(k) == n
                c = R.oor_count(k, lo, hi)
                if hi <= lo:
                    assert c == n  # everything is out
                    continue
                assert c == len(pos) and (n == 0 or c > 0)
                bad = np.flatnonzero((k.astype(np.int64) < lo) | (k.astype(np.int64) >= hi))
                if lay == "one_wave":
                    assert len(np.unique(bad // R.WAVE)) <= 1
                else:
                    assert len(np.unique(bad // R.WAVE)) == len(bad) == -(-n // R.WAVE)
    assert R.oor_count(np.array([R.I32_MAX, R.I32_MIN, 0], np.int32), R.I32_MIN, R.I32_MAX) == 1


def test_exchange_records_round_trip():
    rng = np.random.default_rng(6)
    n = 1000
    ts = rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True)
    term = rng.integers(0, 1 << 31, n).astype(np.int32)
    term[:2] = [0, R.I32_MAX]
    fraud = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
    perm = rng.permutation(n).astype(np.int32)
    rec = R.exchange_pack_ref(ts, term, fraud, perm)
    assert rec.shape == (n, 2) and rec.dtype == np.int64
    # the layout of include/fdx.h, field by field, in plain Python integers
    for j in (0, 1, n - 1):
        r = int(perm[j])
        w = (int(term[r]) << 32) | (int(fraud[r] != 0) << 31) | r
        assert int(rec[j, 0]) == int(ts[r]) and int(rec[j, 1]) == w
    for world in (1, 3, 8):
        t2, loc, fr = R.exchange_unpack_ref(rec, world)
        np.testing.assert_array_equal(t2, ts[perm])
        np.testing.assert_array_equal(loc, term[perm] // world)
        np.testing.assert_array_equal(fr, (fraud[perm] != 0).astype(np.uint8))
    nb = np.array([[0, 5, 1 << 21, 7]], np.int32)
    fr = np.array([[0, 5, 1, 0]], np.int32)
    X = R.reply_assemble_ref(np.full((4, 6), -9.0), R.count_records(nb, fr), np.array([2, 0, 3, 1]), 1)
    np.testing.assert_array_equal(X[[2, 0, 3, 1], 1], [0.0, 5.0, float(1 << 21), 7.0])
    np.testing.assert_array_equal(X[[2, 0, 3, 1], 2], [0.0, 1.0, 1.0 / (1 << 21), 0.0])
    assert (X[:, 0] == -9.0).all() and (X[:, 3:] == -9.0).all()


@pytest.mark.parametrize("W", [1, 2, 3, 4, 7])
def test_rows_case_reaches_its_values(W):
    rng = np.random.default_rng(W)
    d = R.rows_case(W, rng)
    n, nf = d["n"], d["nf"]
    assert n == 4099 and nf == 3 + 4 * W and d["X"].shape == (n, nf)
    assert d["cust_nb"].min() == 0 and d["cust_nb"].max() == 40 and d["tnb"].min() == 0
    assert (np.isnan(d["cust_avg"]) == (d["cust_nb"] == 0)).all() and np.isnan(d["cust_avg"]).any()
    assert ((d["term_risk"] == 0.0) | (d["term_nb"] > 0)).all() and (d["term_risk"] == 1.0).any()
    assert (d["tfr"] <= d["tnb"]).all() and ((d["tnb"] == 0).all(axis=0)).any()
    assert sorted(d["cust_perm"].tolist()) == list(range(n)) and (d["cust_perm"] != d["term_perm"]).any()
    assert not np.isnan(d["amount"]).any()
    np.testing.assert_array_equal(np.round(d["amount"] * 100.0) / 100.0, d["amount"])  # cents
    inv = np.argsort(d["cust_perm"])
    np.testing.assert_array_equal(d["X"][:, 3], d["cust_nb"][0][inv])
    np.testing.assert_array_equal(d["X"][:, 3 + 2 * W], d["tnb"][0])
    dn = R.rows_case(W, rng, nan_variant=True)
    assert 0 < np.isnan(dn["amount"]).sum() <= 9 and (np.isnan(dn["cust_avg"]) & (dn["cust_nb"] > 0)).any()
    mean, scale = R.rows_scaler(nf, rng)
    assert not (np.log2(scale) == np.round(np.log2(scale))).any()


@pytest.mark.parametrize("W,scaled", [(1, False), (3, False), (3, True), (7, True)])
def test_rows_forest_ties_and_nan_step(W, scaled):
    """The thresholds tie with row values, and in the NaN variant missing_go_to_left -- 0 and 1
    mixed on the nodes that split on amount and the customer averages -- decides some leaves: the
    oracle's leaf ids change when it is flipped."""
    rng = np.random.default_rng(10 * W + scaled)
    d = R.rows_case(W, rng, nan_variant=True)
    mean, scale = R.rows_scaler(d["nf"], rng) if scaled else (None, None)
    arr = R.rows_forest(d, rng, mean, scale)
    assert len(arr["node_offsets"]) == 9 and (arr["feature"][arr["left"] >= 0] < d["nf"]).all()
    Z = d["X"] if mean is None else (d["X"] - mean) / scale
    Z32 = Z.astype(np.float32).astype(np.float64)
    ties = sum(int((Z32[:, int(arr["feature"][i])] == arr["threshold"][i]).any()) for i in np.flatnonzero(arr["left"] >= 0))
    assert ties > 10
    feats = [f for f in R.NAN_FEATURES if f < d["nf"] and (f == 0 or f < 3 + 2 * W)]
    nodes, ml = R.nan_split_nodes(arr, feats)
    assert len(nodes) > 0 and 0 < ml.sum() < len(ml)
    _, leaves = oracle.forest_predict(d["X"], arr, mean, scale, want_leaves=True)
    flipped = dict(arr, missing_left=np.where(np.isin(np.arange(len(arr["left"])), nodes), 1 - arr["missing_left"],
                                              arr["missing_left"]).astype(np.uint8))
    _, leaves2 = oracle.forest_predict(d["X"], flipped, mean, scale, want_leaves=True)
    assert (leaves != leaves2).any()
