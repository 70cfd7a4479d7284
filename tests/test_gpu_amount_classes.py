"""Every copy of the pandas roll_sum recurrence on amounts beyond positive cents (amount_classes.py):
signed cents with 0.0 and -0.0, 27 decades of either sign, finite values whose sums overflow,
denormals -- each with and without NaN -- against the C oracle, which test_amount_classes_ref.py
holds equal to pandas on these very inputs.  Compared bit for bit with NaNs canonicalised and
signed zeros distinct (same_bits): assert_array_equal calls -0.0 and 0.0 equal.

  1 k_customer_exact (ops.customer_windows), also on +-inf amounts, and the drop-in on them
  2 k_customer_ring  (customer_layout + customer_windows_interleaved), S = 21, 32, 64
  3 k_customer_walk  (customer_layout(windows_days) + customer_windows_walk)
  4 the strided walk with val_is_avg = 1 (its own division)
  5 scan mode: counts everywhere, averages where prefix sums mean something
  6 FraudPipeline.featurize and run_fused with a FeatureTable; the narrow re-key's cents form
  7 StreamState.update over batch cuts, through a snapshot into other ring sizes

Four segments of every length of amount_classes.LENGTHS plus the escape segment (20.6 k rows): at
3 windows the layout then has a group of the walk's long class (1,500 rows over a 256-row ring),
one of its short class (300 rows over a 128-row ring) and groups of a chunk or less."""
import numpy as np
import pandas as pd
import pytest
import torch

import oracle
from amount_classes import (ESCAPE_POISONED_ROW, ESCAPE_RUN_ROW, FINITE_KINDS, KINDS, PATTERNS, bits, same_bits,
                            segments, table)
from fdx import _lib, ops
from fdx.pipeline import FraudPipeline
from fdx.streaming import StreamState
from table_check import table_as_X

pytestmark = pytest.mark.gpu
REPS = 4
NAN = pytest.mark.parametrize("nan", [False, True], ids=["", "nan"])
PATTERN = pytest.mark.parametrize("pattern", PATTERNS)
FINITE = pytest.mark.parametrize("kind", FINITE_KINDS)
FEATS = ["TX_DURING_WEEKEND", "TX_DURING_NIGHT"] + oracle.CUSTOMER_COLS + oracle.TERMINAL_COLS


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


_SEG, _TAB = {}, {}


def _segments(kind, pattern, nan, windows=(1, 7, 30)):
    """(ts, amt, seg, oracle nb, oracle avg), the oracle run once per input and window set"""
    key = (kind, pattern, nan, windows)
    if key not in _SEG:
        ts, amt, seg = segments(kind, pattern, nan, reps=REPS)
        _SEG[key] = (ts, amt, seg) + tuple(oracle.customer_windows(ts, amt, seg, windows))
    return _SEG[key]


def _table(kind, nan, escape=True):
    """(table, the oracle's [n, 15] feature matrix)"""
    key = (kind, nan, escape)
    if key not in _TAB:
        d = table(kind, "dense", nan, reps=REPS, escape=escape)
        f = oracle.featurize_arrays(d["ts"], d["customer"], d["terminal"], d["amount"], d["fraud"])
        _TAB[key] = (d, np.column_stack([d["amount"]] + [f[k] for k in FEATS]).astype(np.float64))
    return _TAB[key]


# ------------------------------------------------------------------ 1. k_customer_exact
@NAN
@PATTERN
@pytest.mark.parametrize("kind", KINDS)
def test_exact_kernel(dev, kind, pattern, nan):
    for windows in ((1, 7, 30), (2, 5)):
        ts, amt, seg, onb, oavg = _segments(kind, pattern, nan, windows)
        nb, avg = ops.customer_windows(T(ts, torch.int64, dev), T(amt, torch.float64, dev), T(seg, torch.int64, dev),
                                       windows)
        same_bits(nb.cpu().numpy(), onb, f"{kind} {windows} counts")
        same_bits(avg.cpu().numpy(), oavg, f"{kind} {windows} averages")


def _frame(kind, nan):
    ts, amt, seg = segments(kind, "sparse", nan)
    n = len(ts)
    cust = np.repeat(np.arange(len(seg) - 1), np.diff(seg))
    o = np.argsort(ts, kind="stable")
    return pd.DataFrame({"TRANSACTION_ID": np.arange(n), "TX_DATETIME": ts[o].astype("datetime64[ns]"),
                         "CUSTOMER_ID": cust[o], "TERMINAL_ID": np.zeros(n, np.int64), "TX_AMOUNT": amt[o],
                         "TX_FRAUD": np.zeros(n, np.int64)}), (ts, amt, seg)


@NAN
def test_dropin_follows_pandas_on_infinite_amounts(dev, nan):
    """get_customer_spending_behaviour_features claims the pandas contract on arbitrary frames:
    an infinite amount is counted and left out of the sum; scan mode refuses it."""
    from fdx import features

    df, (ts, amt, seg) = _frame("inf", nan)
    out = features.get_customer_spending_behaviour_features(df)
    onb, oavg = oracle.customer_windows(ts, amt, seg)
    same_bits(out["TX_AMOUNT"].values, amt, "rows grouped by customer, in time order")
    for k, w in enumerate((1, 7, 30)):
        same_bits(out[f"CUSTOMER_ID_NB_TX_{w}DAY_WINDOW"].values, onb[k], f"NB {w}")
        same_bits(out[f"CUSTOMER_ID_AVG_AMOUNT_{w}DAY_WINDOW"].values, oavg[k], f"AVG {w}")
    with pytest.raises(ValueError, match="infinite"):
        features.get_customer_spending_behaviour_features(df, mode="scan")


# ------------------------------------------------------- 2.-4. the interleaved layout
def _layout(dev, ts, amt, seg, windows, starts):
    """The layout of _check_interleaved (test_gpu_parity.py): rows reach it through a permutation.
    -> (lay, seg on the device, live-slot mask, grouped position of every live slot)"""
    n = len(ts)
    perm = np.random.default_rng(len(windows)).permutation(n).astype(np.int32)  # grouped position -> "time row"
    ts_time = np.empty_like(ts); ts_time[perm] = ts
    amt_time = np.empty_like(amt); amt_time[perm] = amt
    segd = T(seg, torch.int64, dev)
    lay = ops.customer_layout(segd, T(perm, torch.int32, dev), T(ts_time, torch.int64, dev),
                              T(amt_time, torch.float64, dev), len(windows), windows_days=windows if starts else None)
    irow = lay.irow.cpu().numpy()[: lay.n_slots]
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    real = irow >= 0
    assert real.sum() == n and len(np.unique(irow[real])) == n
    return lay, segd, real, inv[irow[real]]


def _host_avg(sm, nb):
    with np.errstate(all="ignore"):
        return sm / nb  # the consumer's float64 division


@NAN
@PATTERN
@FINITE
def test_ring_kernel(dev, kind, pattern, nan):
    for windows in ((1, 7, 30), (2, 5), (3,)):  # S = 21, 32, 64: the three instantiations
        ts, amt, seg, onb, oavg = _segments(kind, pattern, nan, windows)
        lay, segd, real, g = _layout(dev, ts, amt, seg, windows, starts=False)
        nb, sm = ops.customer_windows_interleaved(lay, segd, windows)
        nb, sm = nb.cpu().numpy()[:, real], sm.cpu().numpy()[:, real]
        same_bits(nb, onb[:, g], f"{kind} {windows} counts")
        same_bits(_host_avg(sm, nb), oavg[:, g], f"{kind} {windows} averages")


def _group_lengths(seg, S=21):
    return np.sort(np.diff(seg))[::-1][::S]


@NAN
@PATTERN
@FINITE
def test_walk_kernel(dev, kind, pattern, nan):
    ts, amt, seg, onb, oavg = _segments(kind, pattern, nan)
    Lg = _group_lengths(seg)
    assert (Lg >= 480).any() and ((Lg > 128) & (Lg < 480)).any() and (Lg <= 16).any()  # both classes, past the rings
    lay, segd, real, g = _layout(dev, ts, amt, seg, (1, 7, 30), starts=True)
    nb, sm = ops.customer_windows_walk(lay, segd)
    nb, sm = nb.cpu().numpy()[:, real], sm.cpu().numpy()[:, real]
    same_bits(nb, onb[:, g], f"{kind} counts")
    same_bits(_host_avg(sm, nb), oavg[:, g], f"{kind} averages")


@NAN
@PATTERN
@FINITE
def test_walk_strided_average(dev, kind, pattern, nan):
    """val_is_avg = 1: the division is the walk's own (its output stage), not the host's."""
    ts, amt, seg, onb, oavg = _segments(kind, pattern, nan)
    lay, segd, real, g = _layout(dev, ts, amt, seg, (1, 7, 30), starts=True)
    m = lay.n_slots
    stride = m + 64
    nb2 = torch.full((3, stride), -77, dtype=torch.int32, device=dev)
    val2 = torch.full((3, stride), -1234.5, dtype=torch.float64, device=dev)
    rc = _lib.load().fdx_customer_windows_walk_strided(
        lay.iamt.data_ptr(), segd.data_ptr(), lay.sorder.data_ptr(), lay.goff.data_ptr(), segd.numel() - 1, m, 3,
        lay.starts.data_ptr(), nb2.data_ptr(), stride, val2.data_ptr(), stride, 1,
        torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "fdx_customer_windows_walk_strided")
    torch.cuda.synchronize()
    nb, avg = nb2.cpu().numpy()[:, :m][:, real], val2.cpu().numpy()[:, :m][:, real]
    want = oavg[:, g]
    same_bits(nb, onb[:, g], f"{kind} counts")
    same_bits(avg, want, f"{kind} averages")
    # what the division must get right is in the data (the oracle's side; the kernel's equals it)
    if kind == "signed":
        assert ((want == 0) & np.signbit(want) & (onb[:, g] > 1)).any(), "-0.0 / n with n > 1"
    if kind == "huge":
        assert np.isinf(want).any()
    if nan:
        assert (np.isnan(want) & (onb[:, g] == 0)).any(), "nb = 0"
    assert bool((nb2[:, m:] == -77).all()) and bool((val2[:, m:] == -1234.5).all())


# ----------------------------------------------------------------------- 5. scan mode
@NAN
@PATTERN
@FINITE
def test_scan_mode(dev, kind, pattern, nan):
    """Counts for every class; averages for cents and signed, at test_gpu_scan.py's tolerance
    (prefix sums of 27 decades or of overflowing values are not meaningful: scan mode is not exact)."""
    ts, amt, seg, onb, oavg = _segments(kind, pattern, nan)
    nb, avg = ops.customer_windows_scan(T(ts, torch.int64, dev), T(amt, torch.float64, dev), T(seg, torch.int64, dev))
    same_bits(nb.cpu().numpy(), onb, f"{kind} counts")
    if kind in ("cents", "signed"):
        a, b = seg[-2], seg[-1]  # (the escape segment overflows: its averages are no prefix differences)
        got, ref = avg.cpu().numpy()[:, :a], oavg[:, :a]
        assert b - a == 55
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-10, atol=1e-9)


# ----------------------------------------------------------------------- 6. pipeline
@pytest.fixture(scope="module")
def forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"]), arrays, z


def _run_pipeline(dev, forest, d, Xo, what, narrow_amounts=0):
    """featurize + score and run_fused with a FeatureTable against the oracle's features and its
    forest on them -> whether the customer re-key's narrow form held (None: not tried)"""
    f, arrays, z = forest
    n = len(d["ts"])
    args = (T(d["ts"], torch.int64, dev), T(d["customer"], torch.int32, dev), T(d["terminal"], torch.int32, dev),
            T(d["amount"], torch.float64, dev), T(d["fraud"], torch.uint8, dev))
    pipe = FraudPipeline(forest=f)
    pipe.narrow_amounts = narrow_amounts
    feats = pipe.featurize(*args, d["n_customers"], d["n_terminals"])
    X = feats.X.cpu().numpy()
    p_feat = pipe.score(feats.X).cpu().numpy()
    rows = ops.FeatureTable(n * 21 + 4096, dev)  # (a lone long customer pads its group of 21)
    rows.buf.fill_(0xAB)
    p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    pipe.run_fused(*args, d["n_customers"], d["n_terminals"], p, rows_out=rows)
    torch.cuda.synchronize()
    Xt = table_as_X(rows, pipe.last_slots, d["amount"])
    same_bits(X, Xo, f"{what}: featurize vs oracle")
    same_bits(Xt, Xo, f"{what}: fused table vs oracle")
    p_ref = oracle.forest_predict(Xo, arrays, z["mean"], z["scale"])
    same_bits(p_feat, p_ref, f"{what}: featurize + score vs the oracle's forest")
    same_bits(p.cpu().numpy(), p_ref, f"{what}: run_fused vs the oracle's forest")
    nf = pipe.narrow_flags[0]
    return None if nf is None or not (nf.mask & _lib.FDX_NARROW_AMOUNT) else nf.holds()


@NAN
@FINITE
def test_pipeline(dev, forest, kind, nan):
    d, Xo = _table(kind, nan)
    assert _run_pipeline(dev, forest, d, Xo, kind) is None
    # with the cents form tried: 1e308 of the escape segment has none, so the re-key falls back for every
    # class here (which class falls back on its own amounts: test_narrow_cents_predicate, no escape segment)
    assert _run_pipeline(dev, forest, d, Xo, f"{kind}, cents tried", narrow_amounts=1) is False


def _without_negative_zero(d):
    keep = ~((d["amount"] == 0) & np.signbit(d["amount"]))
    return {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def test_pipeline_narrow_cents_hold(dev, forest):
    """Tables without the escape segment: cents, and signed cents once the -0.0 rows are gone, travel
    as int32 cents through the re-key and the layout fill, and still give the oracle's bits."""
    for kind in ("cents", "signed"):
        d, _ = _table(kind, False, escape=False)
        if kind == "signed":
            d = _without_negative_zero(d)
            assert (d["amount"] == 0).any() and (d["amount"] < 0).any()
        f = oracle.featurize_arrays(d["ts"], d["customer"], d["terminal"], d["amount"], d["fraud"])
        Xo = np.column_stack([d["amount"]] + [f[k] for k in FEATS]).astype(np.float64)
        assert _run_pipeline(dev, forest, d, Xo, f"{kind} as int32 cents", narrow_amounts=1) is True


@NAN
@FINITE
def test_narrow_cents_predicate(dev, kind, nan):
    """ops.rekey_payload(narrow=True) on tables without the escape segment: the cents form holds for
    cents alone; -0.0 (whose cents would come back as +0.0), NaN, denormals, 1e308 and values of
    other decades fall back, and the grouped amounts keep their bits either way."""
    d, _ = _table(kind, nan, escape=False)
    cases = [(d, kind == "cents" and not nan)]
    if kind == "signed" and not nan:
        cases.append((_without_negative_zero(d), True))
    for t, holds in cases:
        perm, seg, gts, gamt, nar = ops.rekey_payload(T(t["customer"], torch.int32, dev), t["n_customers"],
                                                      T(t["ts"], torch.int64, dev), T(t["amount"], torch.float64, dev),
                                                      narrow=True)
        assert nar.holds() == holds, kind
        p = perm.cpu().numpy()
        np.testing.assert_array_equal(p, np.argsort(t["customer"], kind="stable"))
        same_bits(ops.narrow_unpack(gamt, nar).cpu().numpy(), t["amount"][p], f"{kind} grouped amounts")


# ------------------------------------------------------------------------ 7. streaming
def _update(st, d, a, b, dev):
    return st.update(T(d["ts"][a:b], torch.int64, dev), T(d["customer"][a:b], torch.int32, dev),
                     T(d["amount"][a:b], torch.float64, dev), T(d["terminal"][a:b], torch.int32, dev),
                     T(d["fraud"][a:b], torch.uint8, dev)).cpu().numpy()


@NAN
@FINITE
def test_stream(dev, kind, nan):
    """The state of k_stream_process persists across batches: cuts inside the escape segment's poisoned
    stretch and inside its run of 5.0 must carry nsame through the NaN sum; so must a snapshot taken
    at the first of them, restored into other ring sizes."""
    d, Xo = _table(kind, nan)
    n = len(d["ts"])
    esc = np.flatnonzero(d["customer"] == d["escape"])
    cut_p, cut_r = int(esc[ESCAPE_POISONED_ROW]), int(esc[ESCAPE_RUN_ROW])
    rng = np.random.default_rng(len(kind) + nan)
    cuts = np.unique(np.r_[0, rng.integers(1, n, 10), cut_p, cut_r, n])
    mb = int(np.diff(cuts).max())
    # rings: a customer's 1,500 rows lie inside one 30-day window; a terminal sees ~410 rows in 37 days
    st = StreamState(d["n_customers"], d["n_terminals"], customer_ring=2048, terminal_ring=1024, max_batch=mb)
    X = np.empty((n, 15))
    snap = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == cut_p:
            snap = st.snapshot()
        X[a:b] = _update(st, d, a, b, dev)
    st.check()
    same_bits(X, Xo, f"{kind}: stream vs oracle")
    st2 = StreamState.from_snapshot(snap, customer_ring=4096, terminal_ring=2048, max_batch=mb)
    X2 = np.empty((n - cut_p, 15))
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a >= cut_p:
            X2[a - cut_p:b - cut_p] = _update(st2, d, a, b, dev)
    st2.check()
    np.testing.assert_array_equal(bits(X2), bits(X[cut_p:]), err_msg=f"{kind}: continued from the snapshot")
    np.testing.assert_array_equal(X2.view(np.int64), X[cut_p:].view(np.int64))  # the same device: NaN bits too
